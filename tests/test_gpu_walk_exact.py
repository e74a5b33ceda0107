"""The walk kernels (csrc/diffuse.hip) bit for bit at every state width the launcher branches on.

Inputs and references: tests/walk_exact.py (checked on the host by tests/test_walk_exact_host.py).  Two families of
weights on the same patterns: on the EXACT family every product and sum is exact, so a mismatch with the integer reference
is an indexing or coverage fault (a wrong column, a lost edge, a padding column written, a stale accumulator); on the
ROUNDING family (float32 and float64 weights over 40 binades) only a multiply followed by an add, in the stored order of
the row, the self term last, reproduces the sequential reference.  Every comparison of states and NAMs is for equal bits,
and a failure names the first differing (row, column) and the row's degree.

The engine is driven step by step (ensure_graph, colsums, set_samples, nam_step, nam_full, as
test_gpu_parity.py:test_diffusion_steps_vs_oracle_and_golden does), and through cna.tl.nam and cna.tl.diffuse."""
import functools

import numpy as np
import pandas as pd
import pytest

import walk_exact as wx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


class Case:
    """A pattern with, per family, its matrix and the NAM after every step (the reference state / cells per sample)."""

    def __init__(self, pat, families=wx.FAMILIES, nsteps=wx.NSTEPS):
        self.pat = pat
        self.deg = np.diff(pat.indptr)
        self.C = wx.counts(pat)
        self.fam = {}
        for f in families:
            A = wx.family_matrix(pat, f)
            self.fam[f] = (A, [s / self.C for s in wx.reference_states(pat, f, A, nsteps)])


def same_bits(got, want, case, what):
    msg = wx.first_diff(got, want, case.deg, what)
    assert msg is None, msg


def walk(eng, case, family, kurt=False, expect_sparse=None, check=True):
    """Three steps of the walk on one family's matrix: column sums, the NAM after every step and its padding columns
    against the reference; returns the NAMs and the per-cell kurtosis after every step, and the launches by kernel."""
    pat = case.pat
    A, want = case.fam[family]
    eng.drop_graph()
    eng.ensure_graph(A)
    eng.colsums(1)
    np.testing.assert_array_equal(eng.fetch_colsums(), wx.column_sums(A, 1))
    eng.set_samples(pat.codes, pat.N, case.C)
    eng.prof_reset()
    eng.prof_enable(True)
    nams, kurts = [], []
    nsteps = len(want)
    try:
        for i in range(nsteps):
            eng.nam_step(kurt, i + 1 < nsteps, True)
            got = eng.nam_full()
            nams.append(got)
            what = '%s family, n = %d, N = %d, step %d' % (family, pat.n, pat.N, i + 1)
            if check:
                same_bits(got, want[i], case, what)
            pad = eng.nam_padding()
            assert pad.shape == (pat.n, -pat.N % 4) and not pad.any(), what + ': a padding column is not zero'
            if kurt:
                kurts.append(eng.cell_stat(pat.n))
        eng.sync()
    finally:
        eng.prof_enable(False)
    prof = {k: v[1] for k, v in eng.prof().items()}
    if expect_sparse is not None:
        # (without this a dense walk could be compared with a dense reference and nothing said)
        assert prof.get('nam_first', 0) == 1
        assert prof.get('nam_step_sparse', 0) == (1 if expect_sparse else 0), prof
        assert prof.get('nam_step', 0) == nsteps - 1 - (1 if expect_sparse else 0), prof
    return nams, kurts, prof


# ------------------------------------------------------------------------------------------ a, b, g: the widths
@pytest.fixture(scope='module', params=wx.WIDTH_CASES, ids=lambda c: 'N%d-n%d' % c)
def width_case(request):
    N, n = request.param
    return Case(wx.ladder(n, N, N))


FAMILY = pytest.mark.parametrize('family', wx.FAMILIES)


@FAMILY
def test_widths(eng, width_case, family, monkeypatch):
    """The degree ladder at every width on both sides of every boundary of the launcher's table, n = N + 330 ... cells
    (every residue mod 8; n = N, N + 1, N + 3 at the end of the list): both families after every step, zeros in the
    padding columns, and the compressed second step launched exactly from 96 samples on."""
    monkeypatch.delenv('CNA_SPARSE_MIN_N', raising=False)
    walk(eng, width_case, family, expect_sparse=width_case.pat.N >= wx.SPARSE_MIN_N)


@FAMILY
def test_widths_with_a_dense_second_step(eng, width_case, family, monkeypatch):
    """CNA_SPARSE_MIN_N=0: the second step gathers dense rows too -- every instantiation of k_nam_step (and the
    two-rows-per-wave kernel) on the state a first step leaves -- and gives the same bits."""
    monkeypatch.setenv('CNA_SPARSE_MIN_N', '0')
    walk(eng, width_case, family, expect_sparse=False)


@FAMILY
def test_widths_kurtosis(eng, width_case, family, monkeypatch):
    """The per-cell kurtosis the steps leave on request, against oracle.row_kurtosis of the reference NAM.  (The wave sums
    run in another order: the tolerances of test_diffusion_steps_vs_oracle_and_golden, not bits.)  One sample: every row
    is constant and the kurtosis NaN on both sides, by scipy's rule; from two samples on every reference value is finite,
    so that no NaN stands in for a comparison."""
    from oracle import cna_oracle as orc
    monkeypatch.delenv('CNA_SPARSE_MIN_N', raising=False)
    _, kurts, _ = walk(eng, width_case, family, kurt=True, check=False)
    for k, want in zip(kurts, width_case.fam[family][1]):
        ref = orc.row_kurtosis(want)
        assert np.isnan(ref).all() if width_case.pat.N == 1 else np.isfinite(ref).all()
        np.testing.assert_allclose(k, ref, rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------ c: pair limit, collisions
@functools.lru_cache(maxsize=2)
def pattern_case(kind, N):
    if kind == 'pair_limit':
        return Case(wx.pair_limit(wx.pair_limit_cells(N), N, N))
    if kind == 'collisions':
        return Case(wx.collisions(N + 140, N, N))
    return Case(wx.ladder(N + 331, N, N))


@FAMILY
@pytest.mark.parametrize('kind', ['pair_limit', 'collisions'])
@pytest.mark.parametrize('N', wx.PAIR_LIMIT_N)
def test_pair_limit_and_collisions(eng, N, kind, family, monkeypatch):
    """Rows with 62 ... 65 non-zero samples after the first step (65: the dense row instead of pairs; 65 distinct
    neighbour samples of which one has a stored weight 0.0: still 64 pairs), gathered inside a batch of five, in the ragged
    tail and in a load of 64 edges; rows whose 64 and 130 neighbours all carry one sample.  One N per NQ2 of the
    compressed step."""
    monkeypatch.delenv('CNA_SPARSE_MIN_N', raising=False)
    walk(eng, pattern_case(kind, N), family, expect_sparse=True)


# ------------------------------------------------------------------------------------------ d: row placement
@FAMILY
@pytest.mark.parametrize('N', wx.PLACEMENT_N)
def test_row_placement_and_two_rows_per_wave(eng, N, family, monkeypatch):
    """The ladder on narrow states: in the caller's row order (CNA_REORDER=0: the designed row pairs (300, 0), (33, 1),
    (32, 32), (65, 64) share a wave of k_nam_step_pair), in the device's own order, and with the wave-per-row kernel
    (CNA_STEP_WIDE=1): the same bits; and cna.tl.nam gives them too."""
    import cna_amd as cna
    case = pattern_case('ladder', N)
    monkeypatch.delenv('CNA_SPARSE_MIN_N', raising=False)
    monkeypatch.delenv('CNA_STEP_WIDE', raising=False)
    monkeypatch.setenv('CNA_REORDER', '0')
    walk(eng, case, family, expect_sparse=False)
    assert eng.perm is None
    monkeypatch.delenv('CNA_REORDER')
    walk(eng, case, family, expect_sparse=False)
    monkeypatch.setenv('CNA_STEP_WIDE', '1')
    walk(eng, case, family, expect_sparse=False)
    monkeypatch.delenv('CNA_STEP_WIDE')
    A, want = case.fam[family]
    data = type('D', (), {'obs': pd.DataFrame({'id': case.pat.codes}), 'obsp': {'connectivities': A}, 'uns': {}})()
    NAM, keep = cna.tl.nam(data, 'id', nsteps=wx.NSTEPS, engine=eng)
    assert list(NAM.index) == list(range(N))
    msg = wx.first_diff(NAM.values.T, want[-1][keep], case.deg[keep], 'cna.tl.nam, %s family, N = %d' % (family, N))
    assert msg is None, msg


# ------------------------------------------------------------------------------------- e: the four-byte state
@pytest.mark.parametrize('N', wx.STATE32_N)
def test_four_byte_state_on_exact_inputs(eng, N, monkeypatch):
    """What the walk stores between its steps fits 24 bits on this pattern (test_walk_exact_host.py proves it), so the
    opt-in 4-byte state must give the SAME bits as the 8-byte walk: k_nam_step32h / k_nam_step32 read the right columns.
    With float64 weights on the same pattern the stored step does round, which shows that the option was taken."""
    monkeypatch.delenv('CNA_SPARSE_MIN_N', raising=False)
    case = Case(wx.ladder(wx.width_cells(N), N, N, balanced=True), families=('exact', 'f64'))
    try:
        eng.set_state_f32(True)
        for wide in (False, True):
            if wide:
                monkeypatch.setenv('CNA_STEP32_WIDE', '1')
            else:
                monkeypatch.delenv('CNA_STEP32_WIDE', raising=False)
            walk(eng, case, 'exact', expect_sparse=True)
            nams, _, _ = walk(eng, case, 'f64', expect_sparse=True, check=False)
            want = case.fam['f64'][1]
            same_bits(nams[1], want[1], case, 'f64 family, second step (nothing stored in 4 bytes yet)')
            assert not np.array_equal(nams[2], want[2])
            np.testing.assert_allclose(nams[2], want[2], rtol=3e-7, atol=0)
    finally:
        monkeypatch.delenv('CNA_STEP32_WIDE', raising=False)
        eng.set_state_f32(False)


# ------------------------------------------------------------------------------------------ f: dense diffusion
@FAMILY
@pytest.mark.parametrize('w', [1, 0.25])
def test_dense_diffusion(eng, w, family):
    """cna.tl.diffuse, two steps on 1 ... 1024 columns: the exact family against the integer reference, the other two
    against oracle.diffuse(mode='f64') (and the sequential restatement)."""
    import cna_amd as cna
    from oracle import cna_oracle as orc
    pat = wx.ladder(wx.DENSE_CELLS, 1, 3)
    deg = np.diff(pat.indptr)
    f = family
    A = wx.family_matrix(pat, f, w)
    data = type('D', (), {'obs': pd.DataFrame({'id': pat.codes}), 'obsp': {'connectivities': A}, 'uns': {}})()
    for m in wx.DENSE_M:
        s0 = wx.dense_input(pat, f, m)
        got = cna.tl.diffuse(data, s0.astype(np.float64), 2, self_weight=w, engine=eng)
        want = wx.reference_states(pat, f, A, 2, s0=s0, self_weight=w)[-1]
        what = 'cna.tl.diffuse, %s family, %d columns, self weight %s' % (f, m, w)
        msg = wx.first_diff(got, want, deg, what)
        assert msg is None, msg
        if f != 'exact':
            msg = wx.first_diff(got, orc.diffuse(A, s0, 2, self_weight=w, mode='f64'), deg, what + ' (oracle)')
            assert msg is None, msg

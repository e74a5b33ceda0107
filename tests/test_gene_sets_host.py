"""cna.tl.gene_set_enrich / gene_set_test / cna.ut.read_gmt on the CPU: the matching of the names, the dropped sets, the
choice of the score's sign, nes, p and q, the argument errors -- against an engine double defined here whose
`enrichment_extremes` is the textbook restatement of cna_enrichment_extremes (what the GPU tests compare the device with).

The restatement shares no structure with the kernels: np.argsort(-r, kind='stable') over the valid genes, then a plain
Python walk over all Gv positions that keeps the weight added so far and the misses so far and evaluates
    up_j = S_j / N_R - m_j / (Gv - k)   after every hit,    dn_j = S_(j-1) / N_R - m_j / (Gv - k)   before every hit
(two divisions and a subtraction, the form include/cna_hip.h states, so that dyadic inputs agree with the device to the
bit)."""
import numpy as np
import pandas as pd
import pytest

from test_gene_test_host import restated_bh


# ------------------------------------------------------------------ the restatement (the oracle of the issue)
def restated_extremes(R, set_ptr, set_genes, weight):
    """(up, down, size, valid) as Engine.enrichment_extremes returns them."""
    assert weight in (0, 1, 2)
    R = np.asarray(R, dtype=np.float64)
    n_cols, G = R.shape
    n_sets = len(set_ptr) - 1
    up, down = np.full((n_cols, n_sets), np.nan), np.full((n_cols, n_sets), np.nan)
    size, valid = np.zeros((n_cols, n_sets), dtype=np.int32), np.zeros(n_cols, dtype=np.int32)
    for c in range(n_cols):
        r = R[c]
        ok = np.flatnonzero(np.isfinite(r))
        order = ok[np.argsort(-r[ok], kind='stable')]           # descending, ties in gene order, +0.0 and -0.0 tie
        Gv = len(order)
        valid[c] = Gv
        ranked = r[order]
        w = [float(1.0 if weight == 0 else (abs(x) if weight == 1 else x * x)) for x in ranked]
        for s in range(n_sets):
            member = np.zeros(G, dtype=bool)
            member[np.asarray(set_genes[set_ptr[s]:set_ptr[s + 1]], dtype=np.int64)] = True
            hit = member[order].tolist()
            k = sum(hit)
            size[c, s] = k
            NR = 0.0
            for pos in range(Gv):
                if hit[pos]:
                    NR += w[pos]
            if k == 0 or k == Gv or NR == 0.0:
                continue
            misses = float(Gv - k)
            S, m, hi, lo = 0.0, 0, -np.inf, np.inf
            for pos in range(Gv):
                if hit[pos]:
                    lo = min(lo, S / NR - float(m) / misses)
                    S += w[pos]
                    hi = max(hi, S / NR - float(m) / misses)
                else:
                    m += 1
            up[c, s], down[c, s] = hi, lo
    return up, down, size, valid


class RestatedEngine:
    """The engine as gene_set_enrich sees it."""
    nranks = 1

    def __init__(self):
        self.calls = []

    def enrichment_extremes(self, R, set_ptr, set_genes, weight):
        assert R.dtype == np.float64 and R.flags.c_contiguous and R.ndim == 2
        assert set_ptr.dtype == np.int64 and set_ptr[0] == 0 and set_ptr[-1] == len(set_genes)
        assert set_genes.dtype == np.int32
        for s in range(len(set_ptr) - 1):
            m = set_genes[set_ptr[s]:set_ptr[s + 1]]
            assert (np.diff(m) > 0).all() and (len(m) == 0 or (m[0] >= 0 and m[-1] < R.shape[1]))
        self.calls.append((R.shape, len(set_ptr) - 1, weight))
        return restated_extremes(R, set_ptr, set_genes, weight)


def test_restatement_on_a_case_done_by_hand():
    # six genes, values 5 4 3 2 1 0 -> positions 0..5; the set {0, 3}, weight 1: N_R = 7, two hits, four misses
    #   before hit 1: 0;  after: 5/7;  one miss (position 1), another (2): before hit 2: 5/7 - 2/4;  after: 1 - 2/4;  end 0
    up, down, size, valid = restated_extremes(np.array([[5.0, 4, 3, 2, 1, 0]]), [0, 2], [0, 3], 1)
    assert up[0, 0] == 5.0 / 7.0 and down[0, 0] == 0.0 and size[0, 0] == 2 and valid[0] == 6
    # the set {4, 5} at the bottom: down = 0 - 4/4 before the first hit, up = 1 - 4/4 after the last
    up, down, _, _ = restated_extremes(np.array([[5.0, 4, 3, 2, 1, 1]]), [0, 2], [4, 5], 0)
    assert up[0, 0] == 0.0 and down[0, 0] == -1.0
    # ties keep gene order; a NaN gene has no position; k == Gv, k == 0 and N_R == 0 give NaN
    R = np.array([[1.0, np.nan, 1.0, -0.0, 0.0, np.inf]])
    up, down, size, valid = restated_extremes(R, [0, 1, 3, 7, 9, 11], [2, 1, 5, 0, 2, 3, 4, 3, 4, 0, 1], 1)
    assert valid[0] == 4 and size[0].tolist() == [1, 0, 4, 2, 1]
    assert up[0, 0] == 1.0 - 1.0 / 3.0 and down[0, 0] == -1.0 / 3.0       # gene 2 stands behind gene 0
    assert np.isnan(up[0, 1:4]).all() and np.isnan(down[0, 1:4]).all()
    assert up[0, 4] == 1.0 and down[0, 4] == 0.0


# ------------------------------------------------------------------ gene_set_enrich
GENES = ['g%d' % i for i in range(12)]


def small_case():
    rs = np.random.RandomState(3)
    r = rs.randint(-8, 9, 12) / 8.0
    null_r = rs.randint(-8, 9, (12, 7)) / 8.0
    r[5] = np.nan
    null_r[5] = np.nan
    sets = {'late': ['g9', 'g10', 'g11', 'zzz'], 'tiny': ['g1'], 'early': ['g2', 'g0', 'g1', 'g0'], 'none': ['a', 'b'],
            'nan': ['g5', 'q'], 'wide': GENES[:9]}
    return r, null_r, sets


def test_matching_dropping_and_order():
    import cna_amd as cna
    r, null_r, sets = small_case()
    eng = RestatedEngine()
    out, null_es = cna.tl.gene_set_enrich(r, null_r, sets, GENES, weight=1, min_size=1, max_size=8, return_null=True, engine=eng)
    assert list(out.columns) == ['n_given', 'size', 'es', 'nes', 'p', 'q']
    assert list(out.index) == ['late', 'tiny', 'early', 'nan']             # the dict's order; 'none' (0) and 'wide' (9) dropped
    assert out.attrs['n_dropped'] == 2
    assert out['n_given'].tolist() == [4, 1, 4, 2] and out['size'].tolist() == [3, 1, 3, 0]
    assert eng.calls == [((8, 12), 4, 1)] and null_es.shape == (4, 7)
    # what went to the engine: ascending distinct indices
    R = np.column_stack([r, null_r]).T
    up, down, size, _ = restated_extremes(R, [0, 3, 4, 7, 8], [9, 10, 11, 1, 0, 1, 2, 5], 1)
    es = np.where(up >= -down, up, down)
    assert np.array_equal(out['es'].values, es[0], equal_nan=True) and np.array_equal(null_es, es[1:].T, equal_nan=True)
    assert np.isnan(out.loc['nan', ['es', 'nes', 'p', 'q']].values.astype(float)).all()
    plain = cna.tl.gene_set_enrich(r, null_r, sets, pd.Index(GENES), min_size=1, max_size=8, engine=RestatedEngine())
    assert plain.equals(out)
    # every set dropped: an empty frame, no device call
    eng = RestatedEngine()
    out, null_es = cna.tl.gene_set_enrich(r, null_r, sets, GENES, engine=eng, return_null=True)
    assert len(out) == 0 and out.attrs['n_dropped'] == 6 and eng.calls == [] and null_es.shape == (0, 7)
    assert list(out.columns) == ['n_given', 'size', 'es', 'nes', 'p', 'q']


def test_the_choice_of_the_score():
    from cna_amd.tools._gene_sets import enrichment_scores
    up = np.array([0.5, 0.25, 0.5, np.nan, 0.0])
    down = np.array([-0.25, -0.5, -0.5, np.nan, -1.0])
    assert np.array_equal(enrichment_scores(up, down), [0.5, -0.5, 0.5, np.nan, -1.0], equal_nan=True)   # up == -down: up


def test_nes_p_and_q_by_hand():
    from cna_amd.tools._gene_sets import enrichment_stats
    from cna_amd.tools._gene_test import benjamini_hochberg
    es = np.array([0.5, -0.5, 0.25, np.nan, -0.75, 0.0])
    null = np.array([[0.25, 0.75, -0.5, 0.5],            # three of its sign, mean 0.5; two at least as large
                     [0.25, -0.25, -0.75, np.nan],       # two of its sign (the NaN has none), mean -0.5; one as large
                     [-0.5, -0.25, -1.0, -0.125],        # none of its sign
                     [0.5, 0.5, 0.5, 0.5],
                     [-0.25, -0.5, -0.25, -1.0],         # four, mean -0.5; one as large
                     [0.0, 0.5, -0.5, 0.25]])            # a score of 0 stands with the null scores >= 0: mean 0.25
    nes, p = enrichment_stats(es, null)
    assert np.array_equal(nes[:5], [1.0, -1.0, np.nan, np.nan, -1.5], equal_nan=True) and nes[5] == 0.0
    assert np.array_equal(p, [3 / 4, 2 / 3, 1.0, np.nan, 2 / 5, 1.0], equal_nan=True)
    assert np.array_equal(benjamini_hochberg(p), restated_bh(p), equal_nan=True)
    # ... and through the frame
    import cna_amd as cna
    r, null_r, sets = small_case()
    out, null_es = cna.tl.gene_set_enrich(r, null_r, sets, GENES, min_size=1, max_size=8, return_null=True, engine=RestatedEngine())
    for i, name in enumerate(out.index):
        e, ne = out['es'].values[i], null_es[i]
        if np.isnan(e):
            continue
        same = ne[ne >= 0] if e >= 0 else ne[ne < 0]
        assert out['p'].values[i] == (1.0 + (np.abs(same) >= abs(e)).sum()) / (1.0 + len(same)), name
        if len(same):
            assert abs(out['nes'].values[i] - e / abs(same.mean())) <= 4 * 2.0 ** -52 * abs(out['nes'].values[i]), name
        else:
            assert np.isnan(out['nes'].values[i]) and out['p'].values[i] == 1.0, name
    assert np.array_equal(out['q'].values, restated_bh(out['p'].values), equal_nan=True)


def test_weights_reach_the_engine():
    import cna_amd as cna
    r, null_r, sets = small_case()
    frames = []
    for w in (0, 1, 2):
        eng = RestatedEngine()
        frames.append(cna.tl.gene_set_enrich(r, null_r, sets, GENES, weight=w, min_size=2, max_size=8, engine=eng))
        assert eng.calls == [((8, 12), 2, w)]
    assert not frames[0]['es'].equals(frames[1]['es']) and not frames[1]['es'].equals(frames[2]['es'])


def test_argument_errors():
    import cna_amd as cna
    r, null_r, sets = small_case()
    eng = RestatedEngine()

    def call(**kw):
        args = dict(gene_sets=sets, weight=1, min_size=1, max_size=8)
        args.update(kw)
        return cna.tl.gene_set_enrich(r, null_r, genes=GENES, engine=eng, **args)
    for w in (3, -1, 1.5, '1', True, None):
        with pytest.raises(ValueError, match='weight'):
            call(weight=w)
    with pytest.raises(ValueError, match='min_size'):
        call(min_size=0)
    with pytest.raises(ValueError, match='max_size'):
        call(max_size=4097)
    with pytest.raises(ValueError, match='max_size'):
        call(min_size=5, max_size=4)
    with pytest.raises(ValueError, match='empty'):
        call(gene_sets={})
    with pytest.raises(TypeError, match='dict'):
        call(gene_sets=[('a', ['g1'])])
    with pytest.raises(ValueError, match='one value per gene'):
        cna.tl.gene_set_enrich(r[:-1], null_r, sets, GENES, engine=eng)
    with pytest.raises(ValueError, match='one value per gene'):
        cna.tl.gene_set_enrich(r, null_r[:, 0], sets, GENES, engine=eng)
    with pytest.raises(ValueError, match='unique'):
        cna.tl.gene_set_enrich(r, null_r, sets, GENES[:-1] + ['g0'], engine=eng)
    assert eng.calls == []
    call(max_size=4096)                                       # the device's own limit is allowed


def test_gene_set_test_checks_before_anything_is_queued():
    import cna_amd as cna
    from cna_amd import synth
    from cna_amd.tools import _gene_sets

    class Untouchable:
        nranks = 1

        def __getattr__(self, name):
            raise AssertionError('the engine was asked for %s' % name)
    data, meta = synth.make_dataset(300, 6, k=10, seed=5, builder='cpu')
    data.X = np.zeros((300, 12))
    sets = {'a': GENES[:5]}
    for kw, exc in ((dict(weight=3), ValueError), (dict(min_size=0), ValueError), (dict(max_size=5000), ValueError),
                    (dict(gene_sets={}), ValueError), (dict(gene_sets=None), TypeError)):
        args = dict(gene_sets=sets, engine=Untouchable())
        args.update(kw)
        with pytest.raises(exc):
            cna.tl.gene_set_test(data, meta['y'], 'id', **args)
    # sharded data and a multi-rank engine: refused in the sibling tools' words
    many = Untouchable()
    many.nranks = 2
    with pytest.raises(NotImplementedError, match='does not take sharded data or a multi-rank engine yet'):
        cna.tl.gene_set_test(data, meta['y'], 'id', sets, engine=many)
    assert cna.tl.gene_set_test is _gene_sets.gene_set_test and cna.tl.gene_set_enrich is _gene_sets.gene_set_enrich


def test_gene_set_test_passes_gene_test_through(monkeypatch):
    """gene_test is called unchanged with return_null=True; its frame and attrs come back beside the enrichment."""
    import cna_amd as cna
    from cna_amd.tools import _gene_sets
    r, null_r, sets = small_case()
    genes = pd.DataFrame({'r': r}, index=pd.Index(GENES))
    genes.attrs.update(p=0.125, n_null=7)
    seen = {}

    def fake_gene_test(data, y, sid_name, **kw):
        seen.update(kw, data=data, y=y, sid_name=sid_name)
        return genes, null_r
    monkeypatch.setattr(_gene_sets, 'gene_test', fake_gene_test)
    eng = RestatedEngine()
    out, null_es = cna.tl.gene_set_test('data', 'y', 'id', sets, batches='b', covs='c', donorids='d', layer='L', key_added='k',
                                        min_size=1, max_size=8, return_null=True, engine=eng, Nnull=7, seed=2)
    assert seen == dict(data='data', y='y', sid_name='id', batches='b', covs='c', donorids='d', layer='L', key_added='k',
                        return_null=True, engine=eng, Nnull=7, seed=2)
    want, want_null = cna.tl.gene_set_enrich(r, null_r, sets, GENES, min_size=1, max_size=8, return_null=True, engine=RestatedEngine())
    assert out.equals(want) and np.array_equal(null_es, want_null, equal_nan=True)
    assert out.attrs['p'] == 0.125 and out.attrs['n_null'] == 7 and out.attrs['genes'] is genes and out.attrs['n_dropped'] == 2
    alone = cna.tl.gene_set_test('data', 'y', 'id', sets, min_size=1, max_size=8, engine=eng)
    assert isinstance(alone, pd.DataFrame) and alone.equals(want)


def test_read_gmt(tmp_path):
    import cna_amd as cna
    path = tmp_path / 'sets.gmt'
    path.write_text('HALLMARK_A\thttp://x\tg1\tg2\tg3\n\nB\t\tg2\t\tg9 \r\nC\tonly a description\n')
    sets = cna.ut.read_gmt(str(path))
    assert list(sets) == ['HALLMARK_A', 'B', 'C']
    assert sets == {'HALLMARK_A': ['g1', 'g2', 'g3'], 'B': ['g2', 'g9'], 'C': []}
    bad = tmp_path / 'bad.gmt'
    bad.write_text('A\tx\tg1\nA\ty\tg2\n')
    with pytest.raises(ValueError, match='twice'):
        cna.ut.read_gmt(str(bad))
    bad.write_text('just_a_name\n')
    with pytest.raises(ValueError, match='line 1'):
        cna.ut.read_gmt(str(bad))
    # ... and into the tool
    r, null_r, _ = small_case()
    out = cna.tl.gene_set_enrich(r, null_r, sets, GENES, min_size=2, max_size=8, engine=RestatedEngine())
    assert list(out.index) == ['HALLMARK_A', 'B'] and out.attrs['n_dropped'] == 1

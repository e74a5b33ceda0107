"""cna.tl.coef_raster / cna_coef_raster on the device (run with -m gpu on an MI355X), against the numpy restatement of
tests/test_coef_raster_host.py (itself pinned to np.histogram2d there).

Exact (np.array_equal with equal_nan): extent, n, n_outside, n_pass, top, bottom, covered, absmax -- and sum wherever the
values are dyadic: integers in [-1024, 1024] over 1024, whose sums are exact in any order (fewer than 2^32 cells of
magnitude <= 1 in steps of 2^-10 stay far inside 53 bits).
General float64 values: per pixel |sum_device - sum_restated| <= 2 m 2^-53 sum|v| over the pixel's m passing cells, the
textbook bound (m - 1) u sum|v| (u = 2^-53) for recursive summation in any order, applied to either side."""
import os
import re

import numpy as np
import pytest

from test_coef_raster_host import pixel_index, restated_raster

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ('n', 'n_pass', 'top', 'bottom', 'covered', 'absmax')


def _constant(name):
    src = open(os.path.join(ROOT, 'cna_amd', 'csrc', 'raster.hip')).read()
    return int(re.search(r'constexpr int %s = (\d+);' % name, src).group(1))


SMALL = _constant('RS_SMALL')                  # cells of a pixel that one thread adds up
CHUNK = _constant('RS_CHUNK')                  # cells of a big pixel per wave


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.drop_expression()


def dyadic(rs, *shape):
    return rs.randint(-1024, 1025, size=shape) / 1024.0


def columns_for(n, q, seed, fdr_keys=None):
    """(V, FDR, has_fdr): dyadic values, 5 % NaN, a +inf and a -inf per key (n permitting); every key its own fdr column
    with 5 % NaN; by default the even keys have an fdr."""
    rs = np.random.RandomState(seed)
    V = dyadic(rs, q, n)
    V[rs.rand(q, n) < 0.05] = np.nan
    if n >= 8:
        for k in range(q):
            V[k, (3 + k) % n], V[k, (n - 2 - k) % n] = np.inf, -np.inf
    FDR = rs.rand(q, n) * 0.3
    FDR[rs.rand(q, n) < 0.05] = np.nan
    has = np.array([(k % 2 == 0) if fdr_keys is None else (k in fdr_keys) for k in range(q)], dtype=np.int32)
    return V, FDR, has


def _compare(got, want, tag, exact_sum=True):
    assert got['extent'] == want['extent'], tag
    assert got['n_outside'] == want['n_outside'], tag
    for k in EXACT + (('sum',) if exact_sum else ()):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, '%s %s' % (tag, k)
        assert np.array_equal(got[k], want[k], equal_nan=want[k].dtype == np.float64), '%s %s' % (tag, k)


def _assert_sum_bound(got, want, xy, V, FDR, has, thresh, W, H):
    """|sum_device - sum_restated| <= 2 m 2^-53 sum|v| per pixel and key, m the pixel's passing cells."""
    x0, x1, y0, y1 = want['extent']
    x, y = xy[:, 0], xy[:, 1]
    with np.errstate(invalid='ignore'):
        inside = np.isfinite(x) & np.isfinite(y) & (x0 <= x) & (x <= x1) & (y0 <= y) & (y <= y1)
    for k in range(V.shape[0]):
        with np.errstate(invalid='ignore'):
            ok = inside & np.isfinite(V[k]) & ((FDR[k] <= thresh) if has[k] else True)
        cells = np.flatnonzero(ok)
        p = pixel_index(y[cells], y0, y1, H) * W + pixel_index(x[cells], x0, x1, W)
        absum = np.bincount(p, weights=np.abs(V[k, cells]), minlength=H * W).reshape(H, W)
        assert np.array_equal(np.bincount(p, minlength=H * W).reshape(H, W), want['n_pass'][k])
        bound = 2.0 * want['n_pass'][k] * 2.0 ** -53 * absum
        err = np.abs(got['sum'][k] - want['sum'][k])
        at = np.unravel_index(err.argmax(), err.shape)
        print('key %d: largest error %.3e at a pixel of %d passing cells, its bound %.3e'
              % (k, err[at], want['n_pass'][k][at], bound[at]))
        assert (err <= bound).all()


def _check(eng, xy, V, FDR, has, extent, W, H, radius=0, thresh=0.1, tag=''):
    got = eng.coef_raster(xy, V, FDR, has, thresh, extent, W, H, radius)
    want = restated_raster(xy, V, FDR, has, thresh, extent, W, H, radius)
    _compare(got, want, tag or '%d cells on %d x %d' % (len(xy), W, H))
    return got, want


# ------------------------------------------------------------------ 1. the shapes the kernels branch on
def test_one_cell_on_one_pixel(eng):
    got, _ = _check(eng, np.array([[0.25, -3.0]]), np.array([[0.5]]), None, [0], None, 1, 1)
    assert got['n'][0, 0] == 1 and got['top'][0, 0, 0] == 0.5 and got['extent'] == (-0.25, 0.75, -3.5, -2.5)


@pytest.mark.parametrize('n', [SMALL, SMALL + 1, 63, 64, 65, CHUNK, CHUNK + 1, 2 * CHUNK + 37, 64 * CHUNK + 5])
def test_all_cells_in_one_pixel(eng, n):
    """The thread path up to RS_SMALL cells, then one wave per chunk; beyond 64 chunks the fold's lanes loop."""
    V, FDR, has = columns_for(n, 2, seed=n)
    xy = np.tile([[2.5, 1.5]], (n, 1))
    got, want = _check(eng, xy, V, FDR, has, (0, 4, 0, 4), 4, 4)
    assert want['n'][1, 2] == n and want['n'].sum() == n and 0 < want['n_pass'][1, 1, 2] < n
    _check(eng, xy, V, FDR, has, None, 1, 1)


@pytest.mark.parametrize('H,W', [(1, 7), (7, 1), (65, 63), (67, 130), (4096, 1), (1, 4096)])
def test_grids(eng, H, W):
    """Fewer pixels than one digit of the sort holds, one more digit, partial last digits, the longest sides."""
    rs = np.random.RandomState(H * 7 + W)
    n = 5000
    xy = rs.randn(n, 2) * [1.0, 3.0]
    xy[: n // 2] = xy[: n // 2] * 0.001 + [0.3, -0.7]         # a cluster denser than RS_SMALL per pixel
    V, FDR, has = columns_for(n, 2, seed=H + W)
    got, want = _check(eng, xy, V, FDR, has, None, W, H)
    assert want['n'].sum() == n and want['n'].max() > SMALL
    _check(eng, xy, V, FDR, has, (-1.0, 1.5, -2.0, 2.5), W, H)


def test_the_pixel_limit_with_few_cells(eng):
    rs = np.random.RandomState(5)
    xy = rs.rand(1000, 2)
    V, FDR, has = columns_for(1000, 1, seed=5)
    got, want = _check(eng, xy, V, FDR, has, (0, 1, 0, 1), 2048, 2048)
    assert want['n'].sum() == 1000


# ------------------------------------------------------------------ 2. edges, non-finite coordinates, outside
def test_edges_and_non_finite_coordinates(eng):
    g = np.arange(9.0)
    grid = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)            # every pixel corner of (0, 8, 0, 8) at 8 x 8
    up, down = np.nextafter(8.0, 9.0), np.nextafter(0.0, -1.0)
    odd = np.array([[up, 1.0], [1.0, up], [down, 1.0], [1.0, down], [np.nextafter(8.0, 0.0), np.nextafter(8.0, 0.0)],
                    [np.nan, 1.0], [1.0, np.nan], [np.inf, 1.0], [1.0, -np.inf], [-np.inf, np.inf], [np.nan, np.nan]])
    xy = np.concatenate([grid, odd])
    V, FDR, has = columns_for(len(xy), 2, seed=8)
    got, want = _check(eng, xy, V, FDR, has, (0, 8, 0, 8), 8, 8)
    assert want['n'].sum() == 82 and want['n_outside'] == 4 and want['n'][7, 7] == 5 and want['n'][0, 0] == 1
    auto, _ = _check(eng, xy, V, FDR, has, None, 8, 8)
    assert auto['extent'] == (down, up, down, up) and auto['n_outside'] == 0


def test_every_cell_outside(eng):
    rs = np.random.RandomState(9)
    xy = rs.rand(300, 2) + 5.0
    V, FDR, has = columns_for(300, 2, seed=9)
    got, want = _check(eng, xy, V, FDR, has, (0, 1, 0, 1), 9, 5)
    assert got['n'].sum() == 0 and got['n_outside'] == 300 and np.isnan(got['absmax']).all() and np.isnan(got['top']).all()
    assert (got['sum'] == 0).all()


def test_no_finite_cell(eng):
    xy = np.array([[np.nan, 1.0], [2.0, np.inf]])
    with pytest.raises(ValueError, match='finite coordinates'):
        eng.coef_raster(xy, np.ones((1, 2)), None, [0], 0.1, None, 4, 4)
    _check(eng, xy, np.ones((1, 2)), None, [0], (0, 4, 0, 4), 4, 4)


# ------------------------------------------------------------------ 3. keys and the passing rule
@pytest.mark.parametrize('q', [1, 2, 16])
def test_keys_with_their_own_passing_sets(eng, q):
    rs = np.random.RandomState(q)
    n = 4000
    xy = rs.randn(n, 2)
    V, FDR, has = columns_for(n, q, seed=30 + q, fdr_keys={0, 3, 4, 15})
    got, want = _check(eng, xy, V, FDR, has, None, 33, 17)
    if q > 1:
        assert (want['n_pass'][0] != want['n_pass'][1]).any()
    none, _ = _check(eng, xy, V, None, np.zeros(q, np.int32), None, 33, 17, tag='no key has an fdr')
    assert none['n_pass'].sum() == np.isfinite(V).sum()
    strict, _ = _check(eng, xy, V, FDR, has, None, 33, 17, thresh=0.01)
    assert strict['n_pass'][0].sum() < got['n_pass'][0].sum()


def test_values_that_are_not_finite_count_in_n_only(eng):
    xy = np.tile([[0.5, 0.5]], (6, 1))
    V = np.array([[np.nan, np.inf, -np.inf, 0.25, -0.5, np.nan]])
    got, _ = _check(eng, xy, V, None, [0], (0, 1, 0, 1), 1, 1)
    assert got['n'][0, 0] == 6 and got['n_pass'][0, 0, 0] == 2 and got['sum'][0, 0, 0] == -0.25 and got['absmax'][0] == 0.5
    empty, _ = _check(eng, xy, np.full((1, 6), np.nan), None, [0], (0, 1, 0, 1), 1, 1)
    assert np.isnan(empty['top'][0, 0, 0]) and np.isnan(empty['absmax'][0]) and empty['sum'][0, 0, 0] == 0


# ------------------------------------------------------------------ 4. radius
@pytest.mark.parametrize('radius', [0, 1, 3, 16])
def test_radius_on_a_sparse_grid(eng, radius):
    rs = np.random.RandomState(40)
    n = 60
    xy = rs.rand(n, 2) * [70.0, 45.0]
    xy[:4] = [[0.0, 0.0], [70.0, 45.0], [0.0, 45.0], [35.0, 0.2]]          # discs that cross the border and the corners
    V, FDR, has = columns_for(n, 2, seed=41)
    got, want = _check(eng, xy, V, FDR, has, (0, 70, 0, 45), 70, 45, radius=radius)
    if radius:
        assert want['covered'].sum() > (want['n'] > 0).sum() and np.isfinite(want['top'][0]).sum() > (want['n_pass'][0] > 0).sum()


# ------------------------------------------------------------------ 5. extent, state, determinism
def test_automatic_extent_equals_the_explicit_one_it_implies(eng):
    rs = np.random.RandomState(50)
    xy = rs.randn(3000, 2) * [5.0, 0.01] + [100.0, -1e-3]
    xy[7] = [np.nan, 1e9]
    V, FDR, has = columns_for(3000, 2, seed=50)
    auto, _ = _check(eng, xy, V, FDR, has, None, 40, 30)
    fin = np.isfinite(xy).all(axis=1)
    assert auto['extent'] == (xy[fin, 0].min(), xy[fin, 0].max(), xy[fin, 1].min(), xy[fin, 1].max())
    explicit, _ = _check(eng, xy, V, FDR, has, auto['extent'], 40, 30)
    for k in EXACT + ('sum',):
        assert np.array_equal(auto[k], explicit[k], equal_nan=True), k


def test_a_large_grid_then_a_small_one(eng):
    """The buffers only grow: the second call sees the first one's images and sort tables."""
    rs = np.random.RandomState(60)
    xy = rs.randn(20000, 2)
    V, FDR, has = columns_for(20000, 2, seed=60)
    _check(eng, xy, V, FDR, has, None, 700, 500, radius=2)
    _check(eng, xy[:50] + 0.3, V[:, :50], FDR[:, :50], has, None, 5, 3, radius=1)
    _check(eng, xy[:3000], V[:, :3000], FDR[:, :3000], has, (-1, 1, -1, 1), 64, 64)


def test_general_values_two_runs_and_the_summation_bound(eng):
    rs = np.random.RandomState(70)
    n, H, W = 100000, 65, 63
    xy = rs.randn(n, 2)
    dense = rs.rand(n) < 0.9
    xy[dense] = [0.101, -0.203]                                   # 90 % of the cells in one pixel
    V = rs.randn(2, n)
    V[:, ::17] = np.nan
    FDR = rs.rand(2, n) * 0.2
    has = np.array([1, 0], dtype=np.int32)
    a = eng.coef_raster(xy, V, FDR, has, 0.1, None, W, H)
    eng.coef_raster(xy[:999], V[:, :999], None, [0, 0], 0.1, None, 9, 9)             # another shape in between
    b = eng.coef_raster(xy, V, FDR, has, 0.1, None, W, H)
    for k in EXACT + ('sum',):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    want = restated_raster(xy, V, FDR, has, 0.1, None, W, H)
    _compare(a, want, 'general values', exact_sum=False)
    assert want['n'].max() > 0.85 * n
    _assert_sum_bound(a, want, xy, V, FDR, has, 0.1, W, H)


def test_on_a_context_that_never_saw_a_graph(eng):
    from cna_amd.engine import Engine
    e = Engine(device=0)
    try:
        rs = np.random.RandomState(80)
        V, FDR, has = columns_for(2000, 2, seed=80)
        _check(e, rs.randn(2000, 2), V, FDR, has, None, 50, 20, tag='fresh engine')
        assert e.expression_shape()['format'] == 'none'
    finally:
        e.close()


def test_between_launch_and_fetch_of_a_local_null(eng):
    """coef_raster between cna_null_local_launch and cna_null_local_fetch: the pending pass returns what it returns
    without the call in between, bit for bit, and the images are right."""
    from cna_amd import synth
    from test_gpu_gene_corr import _walk
    N, P = 50, 640
    data, meta = synth.make_dataset(20000, N, k=15, seed=21)
    rs = np.random.RandomState(4)
    y = rs.randn(N)
    y = (y - y.mean()) / y.std()
    Y = np.column_stack([y, rs.randn(N, P)])
    xy = rs.randn(5000, 2)
    V, FDR, has = columns_for(5000, 2, seed=6)
    out = []
    for insert in (False, True):
        eng.null_local_discard()
        eng.drop_graph()
        _walk(eng, data, N)
        nz, maxabs = eng.select_standardized(None, None, y=y)
        maxcorr = max(maxabs, 0.001)
        thr = np.arange(maxcorr / 4, maxcorr, maxcorr / 400)
        edges = thr ** 2 - 1e-8 - 1e-5 * thr ** 2
        eng.condition(np.eye(N), Y)
        eng.null_local_launch(1, P, edges, thr)
        if insert:
            _check(eng, xy, V, FDR, has, None, 90, 70, radius=1, tag='between launch and fetch')
        fetched = eng.null_local_fetch()
        out.append([np.asarray(f).copy() for f in fetched])
    assert len(out[0]) == len(out[1])
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


def test_refusals_leave_the_next_call_right(eng):
    from cna_amd._ffi import CnaHipError
    rs = np.random.RandomState(90)
    xy = rs.randn(1000, 2)
    V, FDR, has = columns_for(1000, 2, seed=90)
    want, _ = _check(eng, xy, V, FDR, has, None, 20, 10)
    for W, H in ((0, 4), (4, 0), (4097, 1), (1, 4097), (2048, 1025)):
        with pytest.raises(CnaHipError, match='width'):
            eng.coef_raster(xy, V, FDR, has, 0.1, None, W, H)
    for radius in (-1, 17):
        with pytest.raises(CnaHipError, match='radius'):
            eng.coef_raster(xy, V, FDR, has, 0.1, None, 4, 4, radius)
    for ext in ((0, 0, 0, 1), (0, 1, 1, 0), (0, np.inf, 0, 1), (np.nan, 1, 0, 1)):
        with pytest.raises(CnaHipError, match='extent'):
            eng.coef_raster(xy, V, FDR, has, 0.1, ext, 4, 4)
    with pytest.raises(CnaHipError, match='q <= 16'):
        eng.coef_raster(xy, np.zeros((17, 1000)), None, np.zeros(17, np.int32), 0.1, None, 4, 4)
    with pytest.raises(ValueError):
        eng.coef_raster(xy[:-1], V, FDR, has, 0.1, None, 4, 4)
    got = eng.coef_raster(xy, V, FDR, has, 0.1, None, 20, 10)
    _compare(got, want, 'after the refusals')


def test_device_memory_returns_after_the_release(eng):
    eng.drop_expression()
    base = eng.device_bytes()
    rs = np.random.RandomState(95)
    xy = rs.randn(3000, 2)
    V, FDR, has = columns_for(3000, 2, seed=95)
    eng.coef_raster(xy, V, FDR, has, 0.1, None, 100, 100, 2)
    grown = eng.device_bytes()
    assert grown - base >= xy.nbytes + V.nbytes + FDR.nbytes
    eng.coef_raster(xy, V, FDR, has, 0.1, None, 100, 100, 2)
    assert eng.device_bytes() == grown                          # grow-only: the same shape allocates nothing
    eng.drop_expression()
    assert eng.device_bytes() == base


# ------------------------------------------------------------------ 6. end to end
def test_after_an_association_on_the_demo_like_dataset(eng):
    import cna_amd as cna
    from cna_amd import synth
    d, samplem = synth.make_demo_like(keep_expression=True)
    cna.tl.association(d, samplem['case'].astype(float), 'id', key_added='coef', Nnull=200, seed=0, engine=eng)
    before = {k: d.obs[k].values.copy() for k in ('coef', 'coef_fdr')}
    G = d.X.shape[1]
    emb = np.stack([d.X[:, :G // 2].mean(axis=1), d.X[:, G // 2:].mean(axis=1)], axis=1).astype(np.float32)
    d.obs['NAMPC1'] = np.random.RandomState(2).randn(len(emb))
    img = cna.tl.coef_raster(d, key=['coef', 'NAMPC1'], basis=emb, shape=(48, 64), radius=1, engine=eng)
    for k, v in before.items():
        assert np.array_equal(d.obs[k].values, v, equal_nan=True), k
    V = np.stack([before['coef'], d.obs['NAMPC1'].values]).astype(np.float64)
    FDR = np.stack([before['coef_fdr'], np.zeros(len(emb))]).astype(np.float64)
    want = restated_raster(emb.astype(np.float64), V, FDR, [1, 0], 0.1, None, 64, 48, 1)
    _compare(img, want, 'demo-like', exact_sum=False)
    passed = np.isfinite(before['coef']) & (before['coef_fdr'] <= 0.1)          # cna.pl.umap_ncorr's mask (_umap.py:10)
    assert int(img['n_pass'][0].sum()) == int(passed.sum()) > 0
    assert img['n'].sum() == len(emb) and img['n_pass'][1].sum() == len(emb)
    assert img['absmax'][0] == np.abs(before['coef'][passed]).max()
    _assert_sum_bound(img, want, emb.astype(np.float64), V, FDR, [1, 0], 0.1, 64, 48)

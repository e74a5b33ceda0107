"""cna.tl.coef_raster on the CPU: the numpy restatement of cna_coef_raster (what the GPU tests compare the device with),
pinned to np.histogram2d off the pixel edges, and the dict, the orientation, the passing rule and the refusals of the host
side against an engine double defined here that records its calls and answers with the restatement."""
import numpy as np
import pandas as pd
import pytest


# ------------------------------------------------------------------ the restatement (the oracle of the issue)
def pixel_index(x, x0, x1, n):
    """The pixel rule along one axis for inside coordinates: t = (x - x0) * s in two roundings, floor; x == x1 and a
    rounded index >= n give n - 1."""
    s = float(n) / (x1 - x0)
    d = x - x0
    t = d * s
    i = np.floor(t).astype(np.int64)
    i[x == x1] = n - 1
    return np.minimum(i, n - 1)


def auto_extent(xy):
    fin = np.isfinite(xy).all(axis=1)
    if not fin.any():
        raise ValueError('coef_raster: no cell has finite coordinates, so there is no extent')
    ext = []
    for a in (0, 1):
        lo, hi = xy[fin, a].min(), xy[fin, a].max()
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5
        ext += [float(lo), float(hi)]
    return tuple(ext)


def disc(r):
    d = np.arange(-r, r + 1)
    return d[:, None] ** 2 + d[None, :] ** 2 <= r * r


def restated_raster(xy, V, FDR, has_fdr, fdr_thresh, extent, width, height, radius=0):
    """What Engine.coef_raster returns, from the definitions of include/cna_hip.h."""
    from scipy import ndimage
    xy = np.asarray(xy, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    q, W, H = V.shape[0], width, height
    x0, x1, y0, y1 = ext = auto_extent(xy) if extent is None else tuple(float(e) for e in extent)
    x, y = xy[:, 0], xy[:, 1]
    fin = np.isfinite(x) & np.isfinite(y)
    with np.errstate(invalid='ignore'):
        inside = fin & (x0 <= x) & (x <= x1) & (y0 <= y) & (y <= y1)
    cells = np.flatnonzero(inside)
    pix = pixel_index(y[cells], y0, y1, H) * W + pixel_index(x[cells], x0, x1, W)
    P = W * H
    out = {'extent': ext, 'n': np.bincount(pix, minlength=P).astype(np.int64).reshape(H, W),
           'n_outside': int((fin & ~inside).sum()), 'n_pass': np.zeros((q, H, W), dtype=np.int64),
           'sum': np.zeros((q, H, W)), 'top': np.full((q, H, W), np.nan), 'bottom': np.full((q, H, W), np.nan),
           'absmax': np.full(q, np.nan)}
    for k in range(q):
        v = V[k, cells]
        ok = np.isfinite(v)
        if has_fdr[k]:
            with np.errstate(invalid='ignore'):
                ok &= np.asarray(FDR, dtype=np.float64)[k, cells] <= fdr_thresh          # a NaN fdr fails
        pk, vk = pix[ok], v[ok]
        out['n_pass'][k] = np.bincount(pk, minlength=P).reshape(H, W)
        out['sum'][k] = np.bincount(pk, weights=vk, minlength=P).reshape(H, W)
        top, bot = np.full(P, -np.inf), np.full(P, np.inf)
        np.maximum.at(top, pk, vk)
        np.minimum.at(bot, pk, vk)
        top, bot = top.reshape(H, W), bot.reshape(H, W)
        if radius > 0:
            top = ndimage.maximum_filter(top, footprint=disc(radius), mode='constant', cval=-np.inf)
            bot = ndimage.minimum_filter(bot, footprint=disc(radius), mode='constant', cval=np.inf)
        out['top'][k] = np.where(np.isinf(top), np.nan, top)
        out['bottom'][k] = np.where(np.isinf(bot), np.nan, bot)
        if vk.size:
            out['absmax'][k] = np.abs(vk).max()
    covered = out['n'] > 0
    if radius > 0:
        covered = ndimage.maximum_filter(covered.astype(np.uint8), footprint=disc(radius), mode='constant', cval=0) > 0
    out['covered'] = covered
    return out


# ------------------------------------------------------------------ the double
class RasterEngine:
    """Records every call; the reduction is `restated_raster`."""

    def __init__(self, nranks=1):
        self.nranks = nranks
        self.calls = []
        self.xy = None

    def coef_raster(self, xy, V, FDR, has_fdr, fdr_thresh, extent, width, height, radius=0):
        self.calls.append(('coef_raster', V.shape[0], list(has_fdr), fdr_thresh, extent, width, height, radius))
        assert xy.dtype == np.float64 and xy.shape == (V.shape[1], 2) and V.dtype == np.float64
        assert FDR is None or (FDR.dtype == np.float64 and FDR.shape == V.shape)
        self.xy = xy
        return restated_raster(xy, V, FDR, has_fdr, fdr_thresh, extent, width, height, radius)


class EmbeddedData:
    """CellData with an obsm."""

    def __init__(self, obs, obsm):
        self.obs, self.obsm = obs, obsm


def _data(obsm=None, **cols):
    from cna_amd.synth import CellData
    n = len(next(iter(cols.values())))
    obs = pd.DataFrame(cols, index=pd.Index(['c%d' % i for i in range(n)]))
    return CellData(obs, None) if obsm is None else EmbeddedData(obs, obsm)


def _cr(*a, **k):
    import cna_amd as cna
    return cna.tl.coef_raster(*a, **k)


def _example(n=500, seed=0):
    rs = np.random.RandomState(seed)
    xy = rs.randn(n, 2) * [2.0, 1.0] + [1.0, -3.0]
    cols = dict(coef=rs.randn(n) * 0.1, coef_fdr=rs.rand(n) * 0.3, NAMPC1=rs.randn(n))
    cols['coef'][rs.rand(n) < 0.1] = np.nan
    return xy, cols


# ------------------------------------------------------------------ the restatement against numpy's own histogram
@pytest.mark.parametrize('W,H', [(8, 8), (16, 4), (5, 7)])
def test_restatement_counts_equal_histogram2d_off_the_edges(W, H):
    """Dyadic coordinates at pixel centres: no rounding, no edge, so both rules must agree."""
    rs = np.random.RandomState(W * 100 + H)
    ix, iy = rs.randint(0, W, 3000), rs.randint(0, H, 3000)
    xy = np.stack([(ix + 0.5) * 0.25 - 1.0, (iy + 0.5) * 0.5 + 2.0], axis=1)
    ext = (-1.0, -1.0 + 0.25 * W, 2.0, 2.0 + 0.5 * H)
    got = restated_raster(xy, np.zeros((1, 3000)), None, [0], 0.1, ext, W, H)
    want = np.histogram2d(xy[:, 1], xy[:, 0], bins=(H, W), range=((ext[2], ext[3]), (ext[0], ext[1])))[0]
    np.testing.assert_array_equal(got['n'], want.astype(np.int64))
    np.testing.assert_array_equal(got['n'], np.bincount(iy * W + ix, minlength=W * H).reshape(H, W))
    assert got['n_outside'] == 0


def test_restatement_counts_equal_histogram2d_on_normal_points():
    xy = np.random.RandomState(3).randn(200000, 2)
    ext = auto_extent(xy)
    got = restated_raster(xy, np.zeros((1, len(xy))), None, [0], 0.1, ext, 64, 64)
    want = np.histogram2d(xy[:, 1], xy[:, 0], bins=(64, 64), range=((ext[2], ext[3]), (ext[0], ext[1])))[0]
    np.testing.assert_array_equal(got['n'], want.astype(np.int64))


def test_restatement_edges_and_dilation():
    xy = np.array([[0., 0.], [8., 8.], [3., 5.], [np.nextafter(8., 9.), 1.], [np.nextafter(0., -1.), 1.], [np.nan, 1.],
                   [1., np.inf]])
    v = np.array([[1., 2., -3., 4., 5., 6., 7.]])
    r = restated_raster(xy, v, None, [0], 0.1, (0, 8, 0, 8), 8, 8)
    assert r['n'][0, 0] == 1 and r['n'][7, 7] == 1 and r['n'][5, 3] == 1 and r['n'].sum() == 3 and r['n_outside'] == 2
    assert r['top'][0, 5, 3] == -3.0 and r['absmax'][0] == 3.0
    d = restated_raster(xy, v, None, [0], 0.1, (0, 8, 0, 8), 8, 8, radius=1)
    assert d['top'][0, 0, 1] == 1.0 and d['top'][0, 1, 0] == 1.0 and np.isnan(d['top'][0, 1, 1])
    assert d['bottom'][0, 5, 4] == -3.0 and d['covered'].sum() == 3 + 3 + 5
    np.testing.assert_array_equal(d['n'], r['n'])
    np.testing.assert_array_equal(d['sum'], r['sum'])


# ------------------------------------------------------------------ the host side
def test_result_keys_shapes_dtypes_and_the_call():
    xy, cols = _example()
    e = RasterEngine()
    img = _cr(_data(**cols), key=['coef', 'NAMPC1'], basis=xy, shape=(6, 9), engine=e)
    assert sorted(img) == ['absmax', 'bottom', 'extent', 'keys', 'mean', 'n', 'n_outside', 'n_pass', 'sum', 'top']
    assert img['keys'] == ['coef', 'NAMPC1'] and isinstance(img['extent'], tuple) and len(img['extent']) == 4
    assert isinstance(img['n_outside'], int) and img['n_outside'] == 0
    assert img['n'].shape == (6, 9) and img['n'].dtype == np.int64 and img['n'].sum() == 500
    assert img['n_pass'].shape == (2, 6, 9) and img['n_pass'].dtype == np.int64
    for k in ('sum', 'mean', 'top', 'bottom'):
        assert img[k].shape == (2, 6, 9) and img[k].dtype == np.float64, k
    assert img['absmax'].shape == (2,) and img['absmax'].dtype == np.float64
    assert e.calls == [('coef_raster', 2, [1, 0], 0.1, None, 9, 6, 0)]
    assert img['extent'] == auto_extent(xy)
    r = _cr(_data(**cols), key='coef', basis=xy, shape=4, radius=2, engine=e)
    assert r['covered'].shape == (4, 4) and r['covered'].dtype == bool and e.calls[-1][-3:] == (4, 4, 2)


def test_orientation_row_is_y_column_is_x():
    xy = np.array([[2.5, 0.5], [0.0, 0.0], [4.0, 2.0]])
    img = _cr(_data(coef=np.array([7.0, np.nan, np.nan])), basis=xy, shape=(2, 4), extent=(0, 4, 0, 2), engine=RasterEngine())
    assert img['n_pass'][0, 0, 2] == 1 and img['n_pass'].sum() == 1 and img['top'][0, 0, 2] == 7.0
    assert img['n'][0, 0] == 1 and img['n'][1, 3] == 1 and img['n'][0, 2] == 1 and img['n'].sum() == 3


def test_mean_is_nan_where_nothing_passes_and_sum_over_count_elsewhere():
    xy, cols = _example()
    img = _cr(_data(**cols), basis=xy, shape=8, engine=RasterEngine())
    none = img['n_pass'] == 0
    assert none.any() and (~none).any()
    assert np.isnan(img['mean'][none]).all() and np.isnan(img['top'][none]).all() and np.isnan(img['bottom'][none]).all()
    assert (img['sum'][none] == 0).all()
    np.testing.assert_array_equal(img['mean'][~none], img['sum'][~none] / img['n_pass'][~none])


def test_passing_rule_with_fdr_without_and_nan_fdr():
    xy = np.zeros((5, 2))
    coef = np.array([1.0, 2.0, 4.0, np.nan, 8.0])
    fdr = np.array([0.05, 0.2, np.nan, 0.01, 0.1])
    e = RasterEngine()
    with_fdr = _cr(_data(coef=coef, coef_fdr=fdr), basis=xy, shape=1, engine=e)
    assert with_fdr['n'][0, 0] == 5 and with_fdr['n_pass'][0, 0, 0] == 2 and with_fdr['sum'][0, 0, 0] == 9.0
    assert with_fdr['top'][0, 0, 0] == 8.0 and with_fdr['bottom'][0, 0, 0] == 1.0 and with_fdr['absmax'][0] == 8.0
    strict = _cr(_data(coef=coef, coef_fdr=fdr), basis=xy, shape=1, fdr_thresh=0.05, engine=e)
    assert strict['n_pass'][0, 0, 0] == 1 and e.calls[-1][3] == 0.05
    without = _cr(_data(coef=coef), basis=xy, shape=1, engine=e)
    assert without['n_pass'][0, 0, 0] == 4 and without['sum'][0, 0, 0] == 15.0 and e.calls[-1][2] == [0]
    assert with_fdr['extent'] == (-0.5, 0.5, -0.5, 0.5)          # the degenerate automatic extent


def test_key_as_str_equals_key_as_list():
    xy, cols = _example()
    a = _cr(_data(**cols), key='coef', basis=xy, shape=8, engine=RasterEngine())
    b = _cr(_data(**cols), key=['coef'], basis=xy, shape=8, engine=RasterEngine())
    both = _cr(_data(**cols), key=['NAMPC1', 'coef'], basis=xy, shape=8, engine=RasterEngine())
    for k in ('n', 'n_pass', 'sum', 'mean', 'top', 'bottom', 'absmax'):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(both['top'][1], a['top'][0])
    np.testing.assert_array_equal(both['n'], a['n'])


def test_basis_in_obsm_components_and_float32():
    xy, cols = _example()
    emb = np.concatenate([xy[:, 1:2], np.zeros((len(xy), 1)), xy[:, 0:1]], axis=1)
    direct = _cr(_data(**cols), basis=xy, shape=8, engine=RasterEngine())
    via = _cr(_data(obsm={'X_umap': emb}, **cols), shape=8, components=(2, 0), engine=RasterEngine())
    for k in ('n', 'top', 'sum'):
        np.testing.assert_array_equal(direct[k], via[k], err_msg=k)
    assert via['extent'] == direct['extent']
    e = RasterEngine()
    x32 = xy.astype(np.float32)
    got = _cr(_data(obsm={'X_umap': x32}, **cols), shape=8, engine=e)
    assert e.xy.dtype == np.float64 and np.array_equal(e.xy, x32.astype(np.float64))
    assert got['extent'] == auto_extent(x32.astype(np.float64))
    with pytest.raises(KeyError):
        _cr(_data(obsm={'X_umap': emb}, **cols), basis='X_tsne', engine=RasterEngine())
    with pytest.raises(KeyError):
        _cr(_data(**cols), engine=RasterEngine())                # the stand-in has no obsm
    with pytest.raises(ValueError, match='components'):
        _cr(_data(obsm={'X_umap': emb}, **cols), components=(0, 3), engine=RasterEngine())
    with pytest.raises(ValueError, match=r'shape \(cells, 2\)'):
        _cr(_data(**cols), basis=emb, engine=RasterEngine())
    with pytest.raises(ValueError, match='coordinates for'):
        _cr(_data(**cols), basis=xy[:-1], engine=RasterEngine())


def test_degenerate_automatic_extent_and_no_finite_cell():
    xy = np.array([[3.0, 1.0], [3.0, 2.0], [np.nan, 9.0]])
    img = _cr(_data(coef=np.ones(3)), basis=xy, shape=2, engine=RasterEngine())
    assert img['extent'] == (2.5, 3.5, 1.0, 2.0) and img['n'].sum() == 2 and img['n_outside'] == 0
    with pytest.raises(ValueError, match='finite coordinates'):
        _cr(_data(coef=np.ones(2)), basis=np.array([[np.nan, 1.0], [2.0, np.inf]]), engine=RasterEngine())


@pytest.mark.parametrize('kw,match', [
    (dict(shape=0), 'height'), (dict(shape=4097), 'height'), (dict(shape=(4, 0)), 'width'), (dict(shape=(4, 4097)), 'width'),
    (dict(shape=2.5), 'height'), (dict(shape=(1, 2, 3)), 'shape'), (dict(shape=2049), r'2\*\*22'),
    (dict(key=['coef', 'NAMPC1'], shape=(2048, 1025)), r'2\*\*22'),
    (dict(radius=-1), 'radius'), (dict(radius=17), 'radius'), (dict(radius=1.5), 'radius'),
    (dict(extent=(0, 0, 0, 1)), 'extent'), (dict(extent=(0, 1, 1, 0)), 'extent'), (dict(extent=(0, np.inf, 0, 1)), 'extent'),
    (dict(extent=(np.nan, 1, 0, 1)), 'extent'), (dict(extent=(0, 1, 0)), 'extent'),
    (dict(key=[]), '1 to 16 keys'), (dict(key=['coef'] * 17), '1 to 16 keys'),
])
def test_refusals_of_values(kw, match):
    xy, cols = _example(50)
    e = RasterEngine()
    with pytest.raises(ValueError, match=match):
        _cr(_data(**cols), **dict(dict(basis=xy), **kw), engine=e)
    assert e.calls == []


def test_limits_are_accepted():
    xy, cols = _example(50)
    e = RasterEngine()
    _cr(_data(**cols), basis=xy, shape=(4096, 1), radius=16, engine=e)
    _cr(_data(**cols), basis=xy, key=['coef'] * 16, shape=(512, 512), engine=e)
    assert [c[1] for c in e.calls] == [1, 16]


def test_refusals_of_keys_and_sharded_data():
    xy, cols = _example(50)
    e = RasterEngine()
    with pytest.raises(KeyError, match='nope'):
        _cr(_data(**cols), key='nope', basis=xy, engine=e)
    with pytest.raises(KeyError, match='NAMPC1_fdr'):
        _cr(_data(**cols), key=['coef', 'NAMPC1'], basis=xy, fdr_thresh=0.1, engine=e)
    with pytest.raises(TypeError, match='not numeric'):
        _cr(_data(coef=np.array(['a'] * 50, dtype=object)), basis=xy, engine=e)
    with pytest.raises(NotImplementedError) as info:
        _cr(_data(**cols), basis=xy, engine=RasterEngine(nranks=2))
    assert info.value.args == ('coef_raster does not take sharded data or a multi-rank engine yet (counts, sums and extremes '
                               'fold over row blocks: a follow-up).',)
    assert e.calls == []


def test_wiring_and_docstring():
    import cna_amd as cna
    from cna_amd import _ffi
    from cna_amd.engine import Engine
    assert 'coef_raster' in cna.tl.__all__
    assert 'cna_coef_raster' in _ffi.SIGNATURES and hasattr(_ffi.load(), 'cna_coef_raster')
    assert callable(Engine.coef_raster)
    doc = cna.tl.coef_raster.__doc__
    assert "ax.imshow(img['n'] > 0, extent=img['extent'], origin='lower', cmap='Greys', alpha=.3)" in doc
    assert "ax.imshow(img['top'][0], extent=img['extent'], origin='lower', cmap='seismic'," in doc

"""The selection pass route against route, at the widths each instantiation of its kernels branches on.

One row pass (csrc/rowstd.h: zero-variance test, centring, optional projector, std with ddof = 1, division, coefficient,
digit planes, max |coefficient|) runs in five layouts: k_select_std (a wave per row), k_select_std16 (16 lanes per row),
the walk's by-product select_tail in the ColPair layout and in the ColQuad layout of the 4-byte state, and
k_selgram_blk.  Two routes to the same X sum a row over the lanes in another order (and the walk does not contract its
products), so they agree to rounding -- 1e-9 relative, the bar of
test_gpu_parity.py::test_selection_as_a_by_product_of_the_last_walk_step, whose assertions these are -- with every
integer identical.  3001 cells: a ragged last group of four rows and a partial last workgroup."""
import warnings

import numpy as np
import pytest

N_CELLS = 3001


def _x_ld(Nx):
    """csrc/c_api.hip:x_ld, restated."""
    ld = (Nx + 3) // 4 * 4
    if ld > 128 and (ld * 8) % 256 == 0 and ld + 4 <= 256:
        ld += 4
    return ld


def test_sixteen_lane_kernel_needs_at_most_four_column_groups():
    """launch_select_std takes k_select_std16<G> up to 256 samples with G = ceil(max(ldx, Kp) / 64) groups of 64 columns,
    Kp the plane width 32 * ceil(Nx / 32): never more than four, so there is no fifth instantiation."""
    for Nx in range(1, 257):
        Kp = 32 * ((Nx + 31) // 32)
        assert -(-max(_x_ld(Nx), Kp) // 64) <= 4, Nx


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    return get_engine()


@pytest.fixture(scope='module')
def eng32():
    from cna_amd.engine import Engine
    e = Engine(device=0)
    e.set_state_f32(True)
    yield e
    e.close()


def _by_product_against_separate_pass(engine, monkeypatch, N):
    import cna_amd as cna
    from cna_amd import synth
    from cna_amd.tools import _association as A
    monkeypatch.setattr(A, '_DEFER_LAST_CELLS', 0)         # (the schedule of large inputs)
    data, meta = synth.make_dataset(N_CELLS, N, k=15, seed=21)
    have = data.obs['id'].nunique()                        # (samples without cells are not part of the NAM)
    assert have == N or (N > 512 and have > 512)           # ... beyond 512 a few are empty: the same instantiations
    out = {}
    for byp in (True, False):
        monkeypatch.setenv('CNA_WALK_SELECT', '1' if byp else '0')
        engine.prof_reset(); engine.prof_enable(True)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res = cna.tl.association(data, meta['y'], 'id', Nnull=130, seed=5, nsteps=3, return_full=True, engine=engine)
        engine.sync(); engine.prof_enable(False)
        out[byp] = (res.p, int(res.k), res.nam.values.copy(), res.kept.copy(), res.fdrs.num_detected.values.copy(),
                    res.ncorrs.values.copy(), res.namresid.values.copy(), res.fdrs.fdr.values.copy(),
                    data.obs['coef'].values.copy(), data.obs['coef_fdr'].values.copy(), res.nullminps.copy(),
                    engine.gram_fetch().copy())
        out[byp, 'select launches'] = engine.prof().get('select', (0, 0))[1]
    assert out[False, 'select launches'] == 1 and out[True, 'select launches'] == 0
    assert out[True][1] == out[False][1]
    # (np.arange(m/4, m, m/400) has 300 or 301 entries depending on the last bits of m: compare the common prefix)
    T = min(len(out[True][4]), len(out[False][4]))
    np.testing.assert_array_equal(out[True][2], out[False][2])                 # NAM
    np.testing.assert_array_equal(out[True][3], out[False][3])                 # kept
    np.testing.assert_array_equal(out[True][4][:T], out[False][4][:T])         # num_detected
    assert out[True][0] == pytest.approx(out[False][0], rel=1e-9)
    for i, (a, b) in enumerate(zip(out[True][5:], out[False][5:])):
        if i == 2:
            a, b = a[:T], b[:T]
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize('N', [66, 130, 250, 256, 260, 520])
def test_by_product_against_the_separate_pass(eng, monkeypatch, N):
    """select_tail<ColPair> of k_nam_step against k_select_std16 / k_select_std.  66: two elements per lane, two column
    groups, ldx 68 beyond one group and a plane width (96) that differs from it; 130: ldx 132, a second pair per lane and a
    ragged last quad of lanes; 250: ldx 252 but planes 256 wide, the fourth group comes from the planes; 256; 260: no
    planes, k_select_std<8>; 520: six pairs per lane with four neighbour rows in flight."""
    _by_product_against_separate_pass(eng, monkeypatch, N)


@pytest.mark.gpu
@pytest.mark.parametrize('N', [66, 130, 250, 260, 520])
def test_by_product_against_the_separate_pass_on_the_four_byte_state(eng32, monkeypatch, N):
    """select_tail<ColQuad>.  66: k_nam_step32h, planes; 130 and 250: k_nam_step32<1>, planes, a ragged last dword;
    260: <2>, no planes; 520: <3>."""
    _by_product_against_separate_pass(eng32, monkeypatch, N)


def _walk(eng, data, nsteps=3):
    """The NAM of `data` resident on the engine; returns its number of samples."""
    from cna_amd.tools._nam import sample_codes
    eng.null_local_discard()
    eng.ensure_graph(data.obsp['connectivities'])
    eng.colsums(1)
    codes, labels = sample_codes(data.obs['id'])
    Ns = len(labels)
    eng.set_samples(codes, Ns, np.bincount(codes, minlength=Ns).astype(float))
    eng.nam_steps(nsteps)
    return Ns


@pytest.mark.gpu
@pytest.mark.parametrize('N,rank,subset', [(60, 2, False), (150, 2, False), (250, 3, False), (300, 1, False), (600, 1, False),
                                           (150, 2, True)])
def test_projector_in_the_selection_pass_against_the_pass_behind_it(eng, N, rank, subset):
    """k_select_std with a projector (and planes up to 256 samples) against select + k_resid_lowrank with centring, the
    division and the coefficients: X and the coefficients to rounding.  One element per lane (60), three (150), four (250),
    eight without planes (300), sixteen (600); and with every seventh cell dropped and the samples reversed."""
    from cna_amd import _ffi, synth
    data, meta = synth.make_dataset(N_CELLS, N, k=15, seed=21)
    Ns = _walk(eng, data)
    assert Ns == N or (N > 512 and Ns > 512)
    rs = np.random.RandomState(N + rank)
    y = rs.randn(Ns)
    y = (y - y.mean()) / y.std()
    Cm = rs.randn(Ns, rank)
    Cm = (Cm - Cm.mean(axis=0)) / Cm.std(axis=0)
    W = np.linalg.solve(Cm.T @ Cm + 1e-3 * Ns * np.eye(rank), Cm.T)
    keep = (np.arange(N_CELLS) % 7 != 0) if subset else None
    colmap = np.arange(Ns, dtype=np.int32)[::-1].copy() if subset else None
    eng.set_resid_factors(Cm, W)
    nz, max_a = eng.select_standardized(keep, colmap, y=y)
    assert nz == 0
    Xa = eng.fetch_matrix(_ffi.MAT_X)
    coef_a = eng.percell()[0].copy()
    eng.clear_resid_factors()
    eng.select(keep, colmap)
    max_b = eng.resid_lowrank(Cm, W, center=True, standardize=True, y=y)
    Xb = eng.fetch_matrix(_ffi.MAT_X)
    coef_b = eng.percell()[0].copy()
    assert Xa.shape == Xb.shape == (N_CELLS if keep is None else int(keep.sum()), Ns)
    np.testing.assert_allclose(Xa, Xb, rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(np.isnan(coef_a), np.isnan(coef_b))
    assert np.isnan(coef_a).sum() == (0 if keep is None else int((~keep).sum()))
    np.testing.assert_allclose(coef_a, coef_b, rtol=1e-9, atol=1e-12)
    assert max_a == pytest.approx(max_b, rel=1e-9)

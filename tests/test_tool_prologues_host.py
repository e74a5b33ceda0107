"""The argument prologue the eight expression-side tools share -- which matrix, which genes, which levels, which numeric
columns, and the refusal of sharded data -- pinned by the full text of every message it raises.

The messages below were recorded from the tools while each of them still carried its own copy of the prologue; they are
compared for equality, so that folding the copies into shared helpers (tools/_genes.py: expression_of, gene_index,
numeric_column; tools/_strata.py: levels_of; tools/_nam.py: refuse_sharded, first_appearance) cannot reword one of them
unnoticed.  One literal differs from that record on purpose: gene_test_strata used to report a missing matrix under
gene_test's name.  CPU only: every message comes before the engine is asked for anything, so the engine is a namespace
with ``nranks`` and nothing else.
"""
import types

import numpy as np
import pandas as pd
import pytest

Y = pd.Series([0.0, 1.0, 2.0])


def _obs():
    return pd.DataFrame({'id': [0, 0, 1, 1, 2, 2], 'cluster': np.array(['b', 'a', None, 'b', 'c', 'a'], dtype=object),
                         'number': [2.0, np.nan, 1.0, 2.0, 3.0, 1.0], 'empty': np.full(6, np.nan),
                         'coef': [0.5, -0.25, 0.0, 1.0, -1.0, 0.125], 'text': np.array(list('uvwxyz'), dtype=object)})


def _data(**attrs):
    return types.SimpleNamespace(obs=_obs(), **attrs)


def _engine(nranks=1):
    return types.SimpleNamespace(nranks=nranks)


def _tools():
    import cna_amd as cna
    return {
        'gene_corr': lambda d, e, strat, key, layer: cna.tl.gene_corr(d, key, layer=layer, engine=e),
        'gene_corr_strata': lambda d, e, strat, key, layer: cna.tl.gene_corr_strata(d, strat, key, layer=layer, engine=e),
        'gene_test': lambda d, e, strat, key, layer: cna.tl.gene_test(d, Y, 'id', layer=layer, engine=e),
        'gene_test_strata': lambda d, e, strat, key, layer: cna.tl.gene_test_strata(d, Y, 'id', strat, layer=layer, engine=e),
        'gene_set_test': lambda d, e, strat, key, layer: cna.tl.gene_set_test(d, Y, 'id', {'s': ['g0']}, layer=layer, engine=e),
        'coef_strata': lambda d, e, strat, key, layer: cna.tl.coef_strata(d, strat, key, engine=e),
        'nam_strata': lambda d, e, strat, key, layer: cna.tl.nam_strata(d, strat, 'id', weights=key, engine=e),
        'expr_to_sample': lambda d, e, strat, key, layer: cna.ut.expr_to_sample(d, 'id', layer=layer, groupby=strat, engine=e),
    }


def _raised(kind, tool, data=None, engine=None, strat='cluster', key='coef', layer=None):
    """The one argument of the exception of type `kind` that the tool raises."""
    with pytest.raises(kind) as info:
        _tools()[tool](data or _data(), engine or _engine(), strat, key, layer)
    assert type(info.value) is kind and len(info.value.args) == 1
    return info.value.args[0]


SHARDED = {
    'gene_corr': 'gene_corr does not take sharded data or a multi-rank engine yet (the per-gene sums add over row blocks: '
                 'one all-reduce away).',
    'gene_corr_strata': 'gene_corr_strata does not take sharded data or a multi-rank engine yet (the per-level sums add over '
                        'row blocks: one all-reduce away).',
    'gene_test': 'gene_test does not take sharded data or a multi-rank engine yet (the per-gene sums add over row blocks: '
                 'one all-reduce away).',
    'gene_test_strata': 'gene_test_strata does not take sharded data or a multi-rank engine yet (the per-level sums add over '
                        'row blocks: one all-reduce away).',
    'gene_set_test': 'gene_set_test does not take sharded data or a multi-rank engine yet (the per-gene sums add over row '
                     'blocks: one all-reduce away).',
    'coef_strata': 'coef_strata does not take sharded data or a multi-rank engine yet (the per-level sums add over row '
                   'blocks, the median and the density need every block: a gather away).',
    'nam_strata': 'nam_strata does not take sharded data or a multi-rank engine yet (the per-level sums add over row blocks: '
                  'an all-reduce away).',
    'expr_to_sample': 'expr_to_sample does not take sharded data or a multi-rank engine yet (the per-row sums add over row '
                      'blocks: one all-reduce away).',
}


@pytest.mark.parametrize('tool', sorted(SHARDED))
def test_sharded_data_and_a_multi_rank_engine_are_refused(tool):
    assert _raised(NotImplementedError, tool, engine=_engine(nranks=2)) == SHARDED[tool]
    part = _data(uns={'cna_shard': {'row0': 0, 'n_global': 12}})
    assert _raised(NotImplementedError, tool, data=part) == SHARDED[tool]


# gene_set_test hands the matrix to gene_test, and says so; gene_test_strata names itself (it used to name gene_test)
MISSING_X = {
    'gene_corr': 'data.X is missing: gene_corr needs the expression matrix',
    'gene_corr_strata': 'data.X is missing: gene_corr_strata needs the expression matrix',
    'gene_test': 'data.X is missing: gene_test needs the expression matrix',
    'gene_test_strata': 'data.X is missing: gene_test_strata needs the expression matrix',
    'gene_set_test': 'data.X is missing: gene_test needs the expression matrix',
    'expr_to_sample': 'data.X is missing: expr_to_sample needs the expression matrix',
}


@pytest.mark.parametrize('tool', sorted(MISSING_X))
def test_a_missing_matrix_and_an_unknown_layer(tool):
    assert _raised(ValueError, tool) == MISSING_X[tool]
    assert _raised(ValueError, tool, data=_data(X=None, layers={'counts': None})) == MISSING_X[tool]
    assert _raised(KeyError, tool, layer='nolayer') == 'nolayer'
    assert _raised(KeyError, tool, data=_data(X=None, layers={'counts': None}), layer='nolayer') == 'nolayer'


ZERO_LEVELS = {
    'gene_corr_strata': "gene_corr_strata: data.obs['empty'] has 0 levels, must lie in [1, 1024]",
    'gene_test_strata': "gene_test_strata: data.obs['empty'] has 0 levels, must lie in [1, 1024]",
    'coef_strata': "coef_strata: data.obs['empty'] has 0 levels, must lie in [1, 1024]",
    'nam_strata': "nam_strata: data.obs['empty'] has 0 levels, must lie in [1, 1024]",
    'expr_to_sample': 'expr_to_sample: 3 samples x 0 levels = 0 rows, must lie in [1, 4096]',      # its own rule: rows
}


@pytest.mark.parametrize('tool', sorted(ZERO_LEVELS))
def test_an_unknown_stratification_and_one_without_levels(tool):
    assert _raised(KeyError, tool, strat='nowhere') == 'nowhere'
    assert _raised(ValueError, tool, strat='empty') == ZERO_LEVELS[tool]


def test_a_missing_stratification_is_reported_before_a_missing_key():
    """Where a tool checks several names before it factorises, the first one it misses is the one it reports."""
    for tool in ('gene_corr_strata', 'coef_strata', 'nam_strata'):
        assert _raised(KeyError, tool, strat='nowhere', key='nokey') == 'nowhere'
        assert _raised(KeyError, tool, key='nokey') == 'nokey'
        assert _raised(KeyError, tool, strat='empty', key='nokey') == 'nokey'           # ... and before the levels are counted
    assert _raised(KeyError, 'gene_corr', key='nokey') == 'nokey'


@pytest.mark.parametrize('tool', ['gene_corr', 'gene_corr_strata', 'coef_strata', 'nam_strata'])
def test_a_key_that_is_not_numeric(tool):
    assert _raised(TypeError, tool, key='text') == "data.obs['text'] is not numeric"
    assert _raised(TypeError, tool, strat='empty' if tool != 'gene_corr' else 'cluster', key='text') \
        == "data.obs['text'] is not numeric"                                            # before the levels are counted


def test_more_than_1024_levels():
    import cna_amd as cna
    many = types.SimpleNamespace(obs=pd.DataFrame({'many': np.arange(1025), 'coef': np.zeros(1025)}))
    with pytest.raises(ValueError) as info:
        cna.tl.coef_strata(many, 'many', engine=_engine())
    assert info.value.args == ("coef_strata: data.obs['many'] has 1025 levels, must lie in [1, 1024]",)


def test_gene_index():
    from cna_amd.tools._genes import gene_index
    names = pd.Index(['g0', 'g1', 'g2'])
    assert gene_index(types.SimpleNamespace(var_names=names), 3) is names
    for data in (types.SimpleNamespace(var_names=names), types.SimpleNamespace(var_names=None), types.SimpleNamespace()):
        index = gene_index(data, 4)
        assert isinstance(index, pd.RangeIndex) and index.equals(pd.RangeIndex(4))


def test_levels_of():
    from cna_amd.tools._strata import levels_of
    obs = _obs()
    codes, levels = levels_of(obs, 'cluster', 'some_tool')
    assert codes.dtype == np.int32 and codes.flags['C_CONTIGUOUS'] and codes.tolist() == [0, 1, -1, 0, 2, 1]
    assert list(levels) == ['b', 'a', 'c']                                              # first appearance; None -> -1
    codes, levels = levels_of(obs, 'number', 'some_tool')
    assert codes.dtype == np.int32 and codes.tolist() == [0, -1, 1, 0, 2, 1] and list(levels) == [2.0, 1.0, 3.0]
    with pytest.raises(KeyError) as info:
        levels_of(obs, 'nowhere', 'some_tool')
    assert info.value.args == ('nowhere',)
    with pytest.raises(ValueError) as info:
        levels_of(obs, 'cluster', 'some_tool', max_levels=2)
    assert info.value.args == ("some_tool: data.obs['cluster'] has 3 levels, must lie in [1, 2]",)

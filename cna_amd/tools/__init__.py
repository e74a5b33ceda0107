"""``cna_amd.tl`` -- same names as the reference's ``cna.tl`` (cna/tools/__init__.py:1-10)."""
from ._nam import nam, svd_nam, diffuse, diffuse_stepwise
from ._association import association
from ._genes import gene_corr
from ._gene_test import gene_test
from ._strata import coef_strata
from ._raster import coef_raster
from ._populations import coef_populations
from ._gene_strata import gene_corr_strata
from ._gene_test_strata import gene_test_strata
from ._gene_markers import gene_markers, gene_markers_pairs, gene_markers_within
from ._gene_rank_corr import gene_rank_corr, gene_rank_corr_strata
from ._gene_rank_perm import gene_rank_test
from ._gene_rank_perm_strata import gene_rank_test_strata
from ._nam_strata import nam_strata
from ._gene_nbhd import gene_nbhd_corr, nbhd_expr
from ._gene_sets import gene_set_enrich, gene_set_test

__all__ = [
    'association',
    'coef_populations',
    'coef_raster',
    'coef_strata',
    'gene_corr',
    'gene_corr_strata',
    'gene_markers',
    'gene_markers_pairs',
    'gene_markers_within',
    'gene_nbhd_corr',
    'gene_rank_corr',
    'gene_rank_corr_strata',
    'gene_rank_test',
    'gene_rank_test_strata',
    'gene_set_enrich',
    'gene_set_test',
    'gene_test',
    'gene_test_strata',
    'nam',
    'nam_strata',
    'nbhd_expr',
    'svd_nam',
    'diffuse',
    'diffuse_stepwise',
]

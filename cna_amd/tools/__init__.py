"""``cna_amd.tl`` -- same names as the reference's ``cna.tl`` (cna/tools/__init__.py:1-10)."""
from ._nam import nam, svd_nam, diffuse, diffuse_stepwise
from ._association import association
from ._genes import gene_corr
from ._gene_test import gene_test

__all__ = [
    'association',
    'gene_corr',
    'gene_test',
    'nam',
    'svd_nam',
    'diffuse',
    'diffuse_stepwise',
]

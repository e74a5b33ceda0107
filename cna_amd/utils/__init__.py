from .multisample import obs_to_sample
from .expression import expr_to_sample
from .gene_sets import read_gmt

__all__ = ['obs_to_sample', 'expr_to_sample', 'read_gmt']

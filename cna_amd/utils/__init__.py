from .multisample import obs_to_sample
from .expression import expr_to_sample

__all__ = ['obs_to_sample', 'expr_to_sample']

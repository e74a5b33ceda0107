"""``cna.tl.gene_set_test`` / ``cna.tl.gene_set_enrich``: gene set enrichment of the per-gene correlations, with the
association's own phenotype permutations as the null.

The reference's demo ends its gene section with the remark that the per-gene correlations to the neighbourhood coefficient
"may be informative on their own, or they could be further analyzed using techniques like gene set enrichment analysis"
(demo/demo.ipynb, section 1.5).  Exporting r to a preranked GSEA permutes genes, which is anti-conservative under gene-gene
correlation.  ``cna.tl.gene_test(..., return_null=True)`` already holds what the phenotype-permutation variant needs: the
correlation of every gene with the coefficient of every permuted phenotype.  The enrichment score of every set under every
column of ``[r | null_r]`` is the device's work (csrc/enrich.hip, ``cna_enrichment_extremes``: a ranking per column, a
running-sum extremum per column and set); this module is the host side only: matching the names, the choice of the score's
sign, the normalisation, the p- and q-values, the frames.
"""
import numpy as np
import pandas as pd

from ..engine import get_engine
from ._gene_test import benjamini_hochberg, gene_test
from ._nam import refuse_sharded

MAX_SET_SIZE = 4096          # members of one set the device takes (csrc/enrich.hip)
COLUMNS = ['n_given', 'size', 'es', 'nes', 'p', 'q']


def _check_arguments(gene_sets, weight, min_size, max_size):
    if not isinstance(gene_sets, dict):
        raise TypeError('gene_sets must be a dict: name -> iterable of gene names')
    if not gene_sets:
        raise ValueError('gene_sets is empty')
    if isinstance(weight, bool) or weight not in (0, 1, 2):
        raise ValueError('weight must be 0, 1 or 2 (the exponent of |r|), not %r' % (weight,))
    if int(min_size) != min_size or min_size < 1:
        raise ValueError('min_size must be an integer >= 1, not %r' % (min_size,))
    if int(max_size) != max_size or max_size > MAX_SET_SIZE:
        raise ValueError('max_size must be an integer <= %d, not %r' % (MAX_SET_SIZE, max_size))
    if max_size < min_size:
        raise ValueError('max_size %r lies below min_size %r' % (max_size, min_size))


def enrichment_scores(up, down):
    """ES = up where up >= -down, else down (NaN where they are)."""
    with np.errstate(invalid='ignore'):
        return np.where(up >= -down, up, down)


def enrichment_stats(es, null_es):
    """-> nes, p of the observed scores es (sets) against null_es (sets x P), each set against the null scores of its own
    sign (a score >= 0 against the null scores >= 0, a score < 0 against those < 0; a NaN null score has no sign):
    nes = es / |mean of them| -- the sign of es is kept --, p = (1 + #{|null| >= |es|}) / (1 + their number).  No null score
    of that sign: nes NaN, p 1.  NaN where es is."""
    es = np.asarray(es, dtype=np.float64)
    null_es = np.asarray(null_es, dtype=np.float64).reshape(len(es), -1)
    with np.errstate(invalid='ignore', divide='ignore'):
        same = np.where((es >= 0)[:, None], null_es >= 0, null_es < 0)
        n_same = same.sum(axis=1)
        mag = np.where(same, np.abs(null_es), 0.0)
        hits = (same & (np.abs(null_es) >= np.abs(es)[:, None])).sum(axis=1)
        nes = np.where(n_same > 0, es / (mag.sum(axis=1) / np.maximum(n_same, 1)), np.nan)
    p = (1.0 + hits) / (1.0 + n_same)
    p[np.isnan(es)] = np.nan
    nes[np.isnan(es)] = np.nan
    return nes, p


def gene_set_enrich(r, null_r, gene_sets, genes, weight=1, min_size=15, max_size=500, return_null=False, engine=None):
    """Phenotype-permutation gene set enrichment of the per-gene correlations ``r`` (one per gene of ``genes``) against
    ``null_r`` (genes x P'), the two results of ``cna.tl.gene_test(..., return_null=True)``.

    ``gene_sets``: dict name -> iterable of gene names.  Names that are not in ``genes`` are dropped (and repeated ones
    counted once); a set whose matched size falls outside [min_size, max_size] is dropped, their number goes to
    ``frame.attrs['n_dropped']``.  ``weight`` 0, 1 or 2 is GSEA's exponent p of the running sum's step |r|^p; other
    exponents are refused, so that host and device agree on every step.  A gene whose r is not finite in a column (a
    constant gene) takes no part in that column.

    Returns a DataFrame indexed by set name in the dict's order: ``n_given`` (names given), ``size`` (matched members that
    are valid in the observed column), ``es`` (the running sum's extreme of larger magnitude; the maximum on a tie),
    ``nes`` = es / |mean of the null es of the same sign|, ``p`` = (1 + #{same-sign null : |es_null| >= |es|}) / (1 +
    #{same-sign null}), ``q`` = Benjamini-Hochberg over the finite p.  es, nes, p and q are NaN for a set without a
    valid member, with every valid gene, or without weight; with no null column of its sign nes is NaN and p is 1.
    ``return_null=True``: ``(frame, null_es)`` with null_es sets x P' float64."""
    _check_arguments(gene_sets, weight, min_size, max_size)
    r = np.asarray(r, dtype=np.float64)
    null_r = np.asarray(null_r, dtype=np.float64)
    index = pd.Index(genes)
    if r.ndim != 1 or null_r.ndim != 2 or null_r.shape[0] != len(r) or len(index) != len(r):
        raise ValueError('gene_set_enrich: r holds one value per gene of `genes`, null_r is genes x permutations')
    if not index.is_unique:
        raise ValueError('gene_set_enrich: the names in `genes` must be unique')
    names, given, members, dropped = [], [], [], 0
    for name, wanted in gene_sets.items():
        wanted = list(wanted)
        at = index.get_indexer(pd.Index(wanted, dtype=object)) if wanted else np.zeros(0, dtype=np.int64)
        at = np.unique(at[at >= 0])                          # ascending and distinct
        if not min_size <= len(at) <= max_size:
            dropped += 1
            continue
        names.append(name)
        given.append(len(wanted))
        members.append(at.astype(np.int32))
    P = null_r.shape[1]
    if names:
        set_ptr = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)
        R = np.ascontiguousarray(np.column_stack([r, null_r]).T)
        engine = engine or get_engine()
        up, down, size, _ = engine.enrichment_extremes(R, set_ptr, np.concatenate(members), int(weight))
        es_all = enrichment_scores(np.asarray(up), np.asarray(down))
        es, null_es = es_all[0], np.ascontiguousarray(es_all[1:].T)
        nes, p = enrichment_stats(es, null_es)
        size = np.asarray(size)[0].astype(np.int64)
    else:
        es = nes = p = np.zeros(0)
        null_es, size = np.zeros((0, P)), np.zeros(0, dtype=np.int64)
    out = pd.DataFrame({'n_given': np.asarray(given, dtype=np.int64), 'size': size, 'es': es, 'nes': nes, 'p': p,
                        'q': benjamini_hochberg(p)}, index=pd.Index(names, dtype=object), columns=COLUMNS)
    out.attrs['n_dropped'] = dropped
    return (out, null_es) if return_null else out


def gene_set_test(data, y, sid_name, gene_sets, batches=None, covs=None, donorids=None, layer=None, key_added='coef', weight=1,
                  min_size=15, max_size=500, return_null=False, engine=None, **kwargs):
    """``gene_test(data, y, sid_name, batches, covs, donorids, layer=layer, key_added=key_added, return_null=True,
    **kwargs)`` unchanged -- the association, ``data.obs[key_added]`` and ``[key_added + '_fdr']``, the per-gene r and its
    null under the association's own permutations -- and then ``gene_set_enrich`` of that (r, null_r) with
    ``data.var_names``: the frame described there, with ``frame.attrs['p']`` the association's global p-value,
    ``frame.attrs['n_null']`` the number of null columns and ``frame.attrs['genes']`` gene_test's own frame.
    ``return_null=True``: ``(frame, null_es)``.  The arguments are checked before anything is queued."""
    _check_arguments(gene_sets, weight, min_size, max_size)
    if 'return_null' in kwargs:
        raise TypeError("gene_set_test() got multiple values for keyword argument 'return_null'")
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'gene_set_test', 'the per-gene sums add over row blocks: one all-reduce away')
    genes, null_r = gene_test(data, y, sid_name, batches=batches, covs=covs, donorids=donorids, layer=layer,
                              key_added=key_added, return_null=True, engine=engine, **kwargs)
    res = gene_set_enrich(genes['r'].values, null_r, gene_sets, genes.index, weight=weight, min_size=min_size,
                          max_size=max_size, return_null=True, engine=engine)
    out, null_es = res
    out.attrs['p'] = genes.attrs['p']
    out.attrs['n_null'] = genes.attrs['n_null']
    out.attrs['genes'] = genes
    return (out, null_es) if return_null else out

/*
 * cna_hip.h -- C ABI of libcna_hip.so: the MI355X (gfx950) hot path of covarying
 * neighborhood analysis (reference: immunogenomics/cna 0.2.3).
 *
 * The reference is pure Python and has no FFI of its own; the boundary a
 * maintainer binds is therefore this library, called from the Python host through ctypes
 * (cna_amd/_ffi.py; INTEGRATION.md shows the stub a reference maintainer would add).
 * Every entry point names the reference lines it replaces (paths under
 * /root/reference/src/cna/tools/).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / numpy types;
 *   - every function returns 0 on success, a hipError_t (>0) or a CNA_E* code (<0) otherwise,
 *     with a human-readable message available from cna_last_error() (thread local);
 *   - the caller owns every host buffer; the library owns all device memory until
 *     cna_ctx_destroy();  one context per host thread; all work is issued on the context's
 *     own HIP stream and entry points that return host data synchronise that stream;
 *   - matrices on the device are "cell-major": one row per cell (neighbourhood), one column
 *     per sample, float64, leading dimension rounded up to a multiple of 4 with zero padding
 *     (the reference's frames are the transpose, samples x cells);
 *   - multi-GPU: one process per GPU; a context owns the contiguous block of graph rows
 *     [row0, row0+n_local) and the same rows of every matrix; sample-space objects are
 *     replicated.  Collectives (RCCL) are internal to the entry points that need them.
 */
#ifndef CNA_HIP_H
#define CNA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cna_ctx cna_ctx;

#define CNA_EINVAL  (-1)   /* bad argument / call order */
#define CNA_ENOMEM  (-2)
#define CNA_ERCCL   (-3)   /* RCCL failure or librccl.so not loadable */
#define CNA_ESTATE  (-4)   /* required earlier step missing */

/* matrix selectors for cna_matrix_shape / cna_fetch_matrix */
#define CNA_MAT_NAM   0    /* NAM after diffusion, all local cells x all samples           */
#define CNA_MAT_X     1    /* working matrix: selected NAM, then residualised NAM in place */
#define CNA_MAT_PROJ  2    /* result of cna_project_keep (cna_fetch_rows only)             */

/* kernel ids for the profiling counters (cna_prof_get) */
enum {
  CNA_K_COLSUM = 0, CNA_K_NAM_FIRST, CNA_K_NAM_STEP, CNA_K_BATCH_KURT, CNA_K_ZEROVAR,
  CNA_K_SELECT, CNA_K_RESID, CNA_K_STANDARDIZE, CNA_K_GRAM, CNA_K_GRAM_REDUCE, CNA_K_NCORRS,
  CNA_K_NULL_LOCAL, CNA_K_OBS_COUNTS, CNA_K_PERCELL_FDR, CNA_K_PROJECT, CNA_K_TRANSPOSE,
  CNA_K_ALLGATHER, CNA_K_CONDITION, CNA_K_GLOBAL_TEST,
  CNA_K_NAM_STEP_SPARSE,        /* the second walk step on the compressed state (k_nam_step_sparse); CNA_K_NAM_STEP is the dense gather */
  /* multi-GPU, so that a scaling run explains itself: CNA_K_ALLGATHER ("rccl") times the collectives of the main
     communicator (all-reduces of column sums / Gram / counts, the all-gather fallback of the state); the two below the
     exchange of state rows between walk steps (pack + ncclSend/Recv + unpack, on its own stream when it overlaps the step)
     and how long the main stream then STOOD STILL waiting for it (0 when the step's safe rows hid it) */
  CNA_K_HALO_EXCHANGE, CNA_K_HALO_WAIT,
  /* cna_matrix_to_bins on the expression stream: the counting sort of the rows with its verdict, then the row list, the
   * sums and the fold (csrc/nam_bins.hip) */
  CNA_K_MATRIX_BINS_SORT, CNA_K_MATRIX_BINS_SUM,
  /* cna_enrichment_extremes on the expression stream: the place of every gene in every column, then the running-sum
   * extremes of every (column, set) (csrc/enrich.hip) */
  CNA_K_ENRICH_POSITIONS, CNA_K_ENRICH_EXTREMES,
  /* cna_expr_cross_by and cna_gram_by on the expression stream: the fill of the level-sorted list, the sums over the cells
   * and their folds; the checks of xrow and the sort's count before them are outside (csrc/expr_cross_by.hip,
   * csrc/gram_by.hip) */
  CNA_K_EXPR_CROSS_BY, CNA_K_GRAM_BY,
  /* cna_coef_raster on the expression stream: the copies of its columns to the device; everything from the extent to the
   * dilated images, its waits for the extent and for the chunk counts included; the copies of the images back
   * (csrc/raster.hip) */
  CNA_K_RASTER_UPLOAD, CNA_K_RASTER, CNA_K_RASTER_FETCH,
  /* cna_graph_components_* on the expression stream: the copy of the classes to the device; per round the hooking of the
   * entries (in the first round three launches -- entry 0 of every row, entry 1, the rest -- with the two flattenings
   * between them), the flattening of the trees and the count of entries that still join two trees (its kernels only:
   * the host's read of that count lies between the rounds); sizes, smallest indices and the compaction of the list; the
   * label kernel; the copies of the list and of the labels back (csrc/components.hip) */
  CNA_K_COMPONENTS_UPLOAD, CNA_K_COMPONENTS_HOOK, CNA_K_COMPONENTS_FLATTEN, CNA_K_COMPONENTS_CHECK, CNA_K_COMPONENTS_TALLY,
  CNA_K_COMPONENTS_LABEL, CNA_K_COMPONENTS_FETCH,
  /* cna_gene_ranksum_by on the expression stream: the keys and levels of a tile of genes; the passes of the radix sort;
   * the rank kernel (in a cna_gene_ranksum_within call: its kernel over the blocks); the copies of the results back
   * (csrc/expr_ranksum.hip) */
  CNA_K_RANKSUM_KEYS, CNA_K_RANKSUM_SORT, CNA_K_RANKSUM_RANK, CNA_K_RANKSUM_FETCH,
  /* cna_gene_ranksum_pairs: the kernel behind the sort (the keys, the sort and the copies back are counted under the ids
   * above) */
  CNA_K_RANKSUM_PAIRS,
  /* cna_gene_rank_corr: the ranks of the columns (their upload, the kept cells, the kernel behind their sort) and the
   * correlation kernel behind the genes' sort; the keys, both sorts and the copies back are counted under
   * CNA_K_RANKSUM_KEYS, _SORT and _FETCH.  cna_gene_rank_corr_x / _x_by / _wide (and cna_x_columns): the kernel that forms the
   * columns from X, or their upload, under CNA_K_RANKCORR_KEYS beside the ranks; the kernel that stores a per entry under
   * CNA_K_RANKSUM_RANK; the dot kernel under CNA_K_RANKCORR_CORR */
  CNA_K_RANKCORR_KEYS, CNA_K_RANKCORR_CORR,
  CNA_K_COUNT
};

/* ---- library / context ------------------------------------------------------------- */
const char* cna_last_error(void);
int  cna_abi_version(void);
int  cna_device_count(int* count);
int  cna_ctx_create(int device, cna_ctx** out);
int  cna_ctx_destroy(cna_ctx* ctx);
int  cna_ctx_sync(cna_ctx* ctx);
/* bytes of device memory currently held by the context */
int  cna_ctx_device_bytes(cna_ctx* ctx, int64_t* bytes);
/* Opt-in storage format of the diffusion state BETWEEN two steps of a walk (reference: the float64 `s` of
   _nam.py:31-34 between iterations of diffuse_stepwise): on != 0 keeps it in 4 bytes per entry from the second step on
   (one rank, more than 64 samples; anything else keeps 8 bytes).  Sums, the NAM and everything after it stay float64;
   the NAM then agrees with the 8-byte walk to ~1e-7 relative instead of bit for bit.  Default off. */
int  cna_set_state_f32(cna_ctx* ctx, int on);

/* ---- multi-GPU (RCCL over xGMI) ------------------------------------------------------ */
/* rank 0 creates a 128-byte id and ships it to the other ranks by any host channel */
int  cna_comm_unique_id(void* id128);
int  cna_comm_init(cna_ctx* ctx, int rank, int nranks, const void* id128);
/* Test communicator: the same collectives staged through a POSIX shared-memory segment `name`
 * (one slot of slot_bytes per rank), so that several ranks can share ONE GPU -- which RCCL refuses --
 * and the multi-rank paths of this library run on a single-GPU box.  Not for production use. */
int  cna_comm_init_shm(cna_ctx* ctx, int rank, int nranks, const char* name, int64_t slot_bytes);
/* which communicator the context holds (0 none, 1 RCCL, 2 the shared-memory test communicator) and the
 * number of ranks as the communicator itself reports it (ncclCommCount) -- bench.py prints both */
int  cna_comm_info(cna_ctx* ctx, int* backend, int* nranks);
/* Start-up check of an RCCL communicator with a time limit per collective: an all-reduce on the main stream, then a
 * ring send / receive on the halo stream's own communicator (cna_comm_init duplicates the communicator for it:
 * the exchange of the diffusion state between steps -- SURVEY.md 8e, the rows of _nam.py:33's s the other ranks
 * need -- runs under the step that produces it) while the main one carries a second all-reduce.  *halo_ok = 0: the
 * halo communicator is absent or did not answer on some rank and was aborted everywhere; exchanges then stay on
 * the main stream.  An error: the main communicator does not work.  No-op without RCCL or with one rank. */
int  cna_comm_selftest(cna_ctx* ctx, double timeout_s, int* halo_ok);

/* Neighbour ("halo") exchange of the diffusion state between steps instead of the all-gather.
 * After cna_graph_upload on every rank: send_rows = LOCAL row indices other ranks need, grouped by
 * destination rank (send_counts[nranks]); recv_rows = GLOBAL row indices this rank's cells
 * reference outside its block, grouped by owner rank (recv_counts[nranks]); the lists of two
 * peers must mirror each other.  NULL counts (and every cna_graph_upload) switch back to the
 * all-gather.  The walk itself is the reference's (_nam.py:31-34); only the data motion differs.
 * With ascending recv_rows that cover every foreign column of the block (the plan of cna_amd._order.halo_plan) the
 * diffusion state then holds n_local + sum(recv_counts) rows instead of n_global -- this rank's rows and, behind them,
 * the rows it receives, which land there directly (a rank owns its rows of A and of S); a block that
 * references a row outside both is refused (CNA_EINVAL).  CNA_COMPACT_STATE=0 keeps the global row space. */
int  cna_set_halo(cna_ctx* ctx, const int64_t* send_rows, const int64_t* send_counts,
                  const int64_t* recv_rows, const int64_t* recv_counts);

/* ---- graph: data.obsp['connectivities'] (_nam.py:12-19,25) ---------------------------- */
/* CSR rows [row0, row0+n_local) of the n_global x n_global kNN graph.  indptr has n_local+1
 * entries rebased so indptr[0]==0; column indices are global.  data is float32 (what scanpy
 * emits) or float64.  Replaces the scipy.sparse object the reference reads. */
int  cna_graph_upload(cna_ctx* ctx, int64_t n_global, int64_t row0, int64_t n_local,
                      const int64_t* indptr, const int32_t* indices,
                      const void* data, int data_is_f64);
/* Optional: the rows handed to cna_graph_upload are a renumbering of the caller's cells (the
 * reference never depends on cell order, _nam.py:25-34; a banded numbering makes the walk's
 * gathers cache-friendly).  orig_index[i] = caller's index of local row i (n_local entries, a
 * slice of one global permutation).  Effect: cna_percell_fdr returns its per-cell outputs in the
 * caller's numbering; every other per-cell array crosses the ABI in library row order.  NULL
 * (and every cna_graph_upload) resets to the identity. */
int  cna_set_cell_order(cna_ctx* ctx, const int64_t* orig_index);
/* The resident graph into another cell order WITHOUT a second trip over PCIe (one rank holding the whole graph, resident
 * in the caller's order): perm[i] = caller's cell that becomes row i (n_global entries, a permutation -- checked).  Same
 * state afterwards as cna_graph_upload of the renumbered rows followed by cna_set_cell_order(perm), except that the column
 * sums and the sample codes are carried over (permuted), not dropped: rows keep the order of their entries, so every
 * result keeps its bits (reference: results do not depend on the order of the cells, _nam.py:25-34). */
int  cna_graph_reorder(cna_ctx* ctx, const int64_t* perm);
/* Sharded callers (one process per GPU, each holding only the cells of its row block -- the layout
 * SURVEY.md 8(e) asks for; the reference has no counterpart, its AnnData is whole): with the local
 * view on, every per-cell array that leaves the library covers this rank's n_local rows only --
 * cna_percell_fdr / _pinned (no all-reduce of cells-sized vectors), the flags of cna_zero_variance,
 * cna_fetch_cell_stat -- and cna_set_cell_order takes indices into the local block.  Sample-space
 * results (Gram, histograms, p-values, medians) stay global.  Call before cna_set_cell_order. */
int  cna_set_local_view(cna_ctx* ctx, int on);
/* colsums = A.sum(axis=0) + self_weight (_nam.py:28), float64, all-reduced over ranks */
int  cna_colsums(cna_ctx* ctx, double self_weight);
int  cna_fetch_colsums(cna_ctx* ctx, double* out_n_global);

/* ---- NAM construction (_nam.py:44-76) ------------------------------------------------ */
/* codes[i] = column of cell i in pd.get_dummies(obs[sid]) (_nam.py:51), for ALL n_global cells;
 * counts[c] = cells per sample C (_nam.py:54). */
int  cna_set_samples(cna_ctx* ctx, const int32_t* codes, int n_samples, const double* counts);
/* start a new walk from the one-hot state with the sample codes already on the device (same
 * effect as calling cna_set_samples again with identical arguments, without the upload) */
int  cna_restart_nam(cna_ctx* ctx);
/* One diffusion step s <- A.(s/colsums) + w*s/colsums (_nam.py:31-34) of the sample indicators.
 * The first call after cna_set_samples starts from the one-hot matrix.
 *   want_kurt : also produce per-cell kurtosis over samples of s/C (_nam.py:59), readable with
 *               cna_fetch_cell_stat;
 *   may_continue : keep the scaled state for another step (exchanged across ranks);
 *   may_stop  : also write NAM = s/C (_nam.py:73) so the walk can end here. */
int  cna_nam_step(cna_ctx* ctx, int want_kurt, int may_continue, int may_stop);
/* nsteps steps with a fixed step count and no per-step host decision (nsteps given, no progress
 * output): cna_nam_step(0, more, last) x nsteps in one call */
int  cna_nam_steps(cna_ctx* ctx, int nsteps);
/* A hint for the walk in progress: y[0..n_samples) is the standardised phenotype that the analysis will hand to
 * cna_select_standardized[_fused] with every cell and every sample kept and nothing to regress out
 * (_association.py:182,77; _nam.py:122,159).  The next cna_nam_step that ends its walk (may_continue = 0) then leaves,
 * besides the NAM, what that call computes from it -- X, its digit planes, the coefficients X.y/N, the zero-variance
 * count -- and the call finds its pass done (its results agree with the separate pass to rounding: the row sums run
 * over the lanes in another order).  Wide sample axes only (more than 64 samples); y = NULL clears; a selection call
 * that asks for anything else simply runs its own pass from the NAM. */
int  cna_nam_select_hint(cna_ctx* ctx, const double* y, int n_samples);
/* per-cell statistic of the last kernel that produced one (kurtosis / batch kurtosis),
 * gathered over ranks: out has n_global entries (CNA_MAT_NAM rows) or n_x_total (CNA_MAT_X) */
/* The whole walk of _nam.py:57-70 with nsteps=None in one call: steps are taken until the median over the cells of
 * the per-cell kurtosis (np.median, _nam.py:59) falls by less than 3 from one step to the next (checked from the
 * third step on, _nam.py:64-68), at most maxnsteps (<= 16).  The medians and the rule are evaluated on the device
 * and steps are queued ahead of the verdict (those behind the last step return at once); the host reads one word
 * per batch of steps.  *steps_out: steps taken; medkurt_out (maxnsteps doubles, may be NULL): the median after
 * every step taken.  Leaves the NAM of the last step on the device, like cna_nam_step(.., may_stop=1). */
int  cna_nam_auto(cna_ctx* ctx, int maxnsteps, int* steps_out, double* medkurt_out);
/* The same in two halves: _launch queues the first four steps with their medians and the rule and returns at once (the
 * host goes on with its own work); _finish reads the verdict, queues two more steps at a time while the rule is not met,
 * and leaves the context as cna_nam_auto does.  Every entry point that reads or replaces the NAM finishes a pending
 * walk itself, so calling _finish is only needed for its outputs. */
int  cna_nam_auto_launch(cna_ctx* ctx, int maxnsteps);
int  cna_nam_auto_finish(cna_ctx* ctx, int* steps_out, double* medkurt_out);
/* _qc_nam's decision (_nam.py:94-96) on the statistic left by cna_batch_kurtosis(CNA_MAT_NAM, ...): np.median of it,
 * threshold = max(6, 2 median), and the number of cells that fail `kurtosis < threshold` (NaN fails) -- 0 means every
 * cell is kept and the per-cell vector need not be fetched (cna_fetch_cell_stat).  Median, threshold and count are
 * formed on the device; one wait. */
int  cna_stat_qc(cna_ctx* ctx, double* median_out, double* threshold_out, int64_t* n_dropped_out);
int  cna_fetch_cell_stat(cna_ctx* ctx, double* out, int64_t n_expected);
/* np.median of that statistic over all cells (or all kept cells, all ranks), computed on the device
 * by an exact radix select: NaN if any entry is NaN, mean of the two middle values for an even count
 * (medians of _nam.py:59,94,150) */
int  cna_stat_median(cna_ctx* ctx, double* median_out);
/* FOR TESTS.  The analysis never calls this: it exists so that the suite can choose, bit by bit, the vector that
 * cna_stat_median, cna_stat_qc and cna_fetch_cell_stat work on (the reference's medians and QC count: _nam.py:64-68,
 * _nam.py:94-96), where the kurtosis kernels only ever leave a narrow band of values.  v[0..n) replaces the NAM-space
 * per-cell statistic as it stands on the device (device cell order; medians and counts do not depend on the order).
 * One rank holding the whole graph; n must equal n_global (CNA_EINVAL, as for v = NULL); CNA_ESTATE before
 * cna_graph_upload, on a sharded context, and while a local-null pass is pending. */
int  cna_load_cell_stat(cna_ctx* ctx, const double* v, int64_t n);

/* cna.tl.diffuse / diffuse_stepwise on an arbitrary dense cells x m state (_nam.py:21-41):
 * load the local rows, step, fetch the local rows (unscaled state s). */
int  cna_dense_load(cna_ctx* ctx, const double* s_local, int m);
int  cna_dense_step(cna_ctx* ctx);
int  cna_dense_fetch(cna_ctx* ctx, double* s_local_out);

/* ---- QC / selection (_nam.py:78-99, _association.py:175-191) --------------------------- */
/* _batch_kurtosis (_nam.py:78-82) of matrix `which`: per cell, Pearson kurtosis over the
 * per-batch means; batch_codes[s] in [0,n_batches) per column of that matrix. */
int  cna_batch_kurtosis(cna_ctx* ctx, int which, const int32_t* batch_codes, int n_batches);
/* cells whose NAM entries are constant over the selected samples (NAM.std(axis=0)==0,
 * _association.py:182): flags (1 byte per cell, all n_global cells, gathered over ranks) and
 * their total number. colmap NULL = all samples. */
int  cna_zero_variance(cna_ctx* ctx, const int32_t* colmap, int n_sel, uint8_t* flags_out,
                       int64_t* n_zero_out);
/* X[i', c'] = NAM[keep_idx[i'], colmap[c']]  (NAM.reindex(y.index)[filter], iloc[:, keep], drop;
 * _nam.py:99, _association.py:178-185).  keep_idx: local row indices, NULL = all rows. */
int  cna_select(cna_ctx* ctx, const int64_t* keep_idx, int64_t n_keep,
                const int32_t* colmap, int n_sel);
/* cna_select followed by centring and division by the per-cell std (ddof=1) in one pass, for the
 * case M = I (_association.py:178-185 + _nam.py:122,159); n_zero_out = number of selected cells with
 * zero variance over the selected samples, summed over ranks (if non-zero the caller drops them
 * with cna_zero_variance + cna_select and standardises again).  With y (n_sel doubles, the
 * standardised phenotype in X's column order) the rows are final when they leave the kernel, so
 * cna_ncorrs(y) is taken in the same pass: max_abs_out = max |ncorrs| over all ranks. */
/* one-shot: the next cna_select_standardized[_fused] over N selected samples also applies M = I - C.W
 * (factors as in cna_resid_lowrank; _nam.py:128-135) between the centring and the division by the std */
int  cna_set_resid_factors(cna_ctx* ctx, const double* C, const double* W, int r, int N);
/* cna_select plus, in the same pass, the number of selected cells whose selected entries have zero variance
 * (_association.py:182-185); non-zero: the caller redoes the step with cna_zero_variance + cna_select */
int  cna_select_checked(cna_ctx* ctx, const int64_t* keep_idx, int64_t n_keep, const int32_t* colmap, int n_sel,
                        int64_t* n_zero_out);
int  cna_select_standardized(cna_ctx* ctx, const int64_t* keep_idx, int64_t n_keep,
                             const int32_t* colmap, int n_sel, int64_t* n_zero_out,
                             const double* y /* or NULL */, double* max_abs_out /* or NULL */);
/* The same, plus -- when no selected cell has zero variance -- what the host would queue next from
 * values it has to wait for here anyway: the Gram kernels (cna_gram_launch), the local null's
 * thresholds np.arange(m/4, m, m/400) from m = max|ncorrs| (returned in thr_out[<= 512], *T_out of
 * them; _association.py:101), cna_null_local_prepare(null_P, edges(thr), thr) and
 * cna_percell_coef_launch.  *T_out = 0: only the selection (and possibly the Gram) was issued.
 * null_col0 >= 0: the conditioned phenotypes of this analysis are resident already -- the caller vouches for it
 * (null_flag NULL: cna_condition_phenotypes has returned), or *null_flag == 1 at the moment the pass could start
 * (cna_host_draw_then_condition sets it); the prepared pass is then launched on columns null_col0 ... as
 * cna_null_local_launch(ctx, null_col0, null_P, NULL, T, 0, NULL) would, *null_launched = 1. */
int  cna_select_standardized_fused(cna_ctx* ctx, const int64_t* keep_idx, int64_t n_keep, const int32_t* colmap,
                                   int n_sel, int64_t* n_zero_out, const double* y, double* max_abs_out,
                                   int null_P, int* T_out, double* thr_out, int* gram_queued, int* coef_queued,
                                   int null_col0, const int* null_flag, int* null_launched);
/* numpy's thresholds / bin edges of the local null for a given max|ncorrs| (host arithmetic only) */
int  cna_reference_thresholds(double maxabs, int cap, double* thr, double* edges);
/* upload a cells x samples matrix as X (cna.tl.svd_nam on a user NAM, _nam.py:102) */
int  cna_upload_x(cna_ctx* ctx, const double* x_local, int64_t n_rows, int n_cols);

/* ---- residualisation + PCA (_nam.py:102-177) ------------------------------------------ */
/* X <- (X - rowmean(X))  if center  (_nam.py:122);  then X <- X . M^T if M != NULL
 * (_nam.py:135,148; M is n_cols x n_cols row-major). */
int  cna_resid_apply(cna_ctx* ctx, const double* M, int center);
/* X <- X / std(X over samples, ddof=1)  (_nam.py:159); center!=0 subtracts the mean first
 * (svd_nam's own re-standardisation, _nam.py:103-104). */
/* the same residualisation for a projector given by its factors, M = I - C.W (C: N x r standardised batches /
 * covariates, W = (C^T C + ridge N L)^-1 C^T: r x N, _nam.py:128-148): x.M^T = x - (x.W^T).C^T row by row, fused
 * with the centring (_nam.py:122) and optionally the division by the std (_nam.py:159) and the neighbourhood
 * coefficients X.y/N with their max |.| (_association.py:77,101): one pass over X instead of three */
int  cna_resid_lowrank(cna_ctx* ctx, const double* C, const double* W, int r, int center, int standardize,
                       const double* y, double* max_abs_out);
/* One ridge of the schedule of _nam.py:142-156 in one pass over X and one wait: centre, apply M = I - C.W (factors as
 * above), take the batch kurtosis of the result (_nam.py:150; batch_codes: batch of every sample of X, -1 = none) and
 * its np.median (on the device, *median_out), and -- optimistically -- divide by the std (_nam.py:159) and take the
 * coefficients X.y/N (_association.py:77; *max_abs_out = max |coefficient|).  median <= 6: the schedule is over and X is
 * final.  Otherwise X has to be restored by the caller (cna_select_checked from the NAM) before the next ridge. */
int  cna_resid_lowrank_bk(cna_ctx* ctx, const double* C, const double* W, int r, const double* y, double* max_abs_out,
                          const int32_t* batch_codes, int n_batches, double* median_out);
/* Selection, QC and the first ridge of the demo's call shape (covariates AND batches, demo/demo.ipynb:149) in ONE pass over
 * the NAM: what cna_batch_kurtosis(CNA_MAT_NAM) + cna_stat_qc (_nam.py:85-99), cna_select_checked with every cell and every
 * sample in place (_association.py:178-185) and cna_resid_lowrank_bk (_nam.py:136-159, first ridge) compute in three passes.
 * At most seven batches (the kurtosis of so few batch means cannot reach 6: a row fails the QC only with a NaN kurtosis), no
 * sample without a batch, at most 128 samples.  Out: *n_qc_failed rows with a NaN batch kurtosis, *n_zero rows constant over
 * the samples, *median_out / *max_abs_out as cna_resid_lowrank_bk.  When both counts are 0 and the median is <= 6, X is final;
 * otherwise the caller runs the three calls (the NAM is untouched).  *done = 0: shape not covered, nothing queued. */
int  cna_select_resid_bk(cna_ctx* ctx, const double* C, const double* W, int r, const double* y, double* max_abs_out,
                         const int32_t* batch_codes, int n_batches, double* median_out, int64_t* n_qc_failed,
                         int64_t* n_zero, int* done);
int  cna_standardize(cna_ctx* ctx, int center);
/* G = X^T X over all cells of all ranks (NAM.dot(NAM.T), _nam.py:105), n_cols x n_cols row-major */
int  cna_gram(cna_ctx* ctx, double* G_out);
/* the same in two halves: queue the kernels, collect the matrix later (the copy does not wait
 * for work queued after the launch, e.g. the local-null kernel) */
int  cna_gram_launch(cna_ctx* ctx);
int  cna_gram_fetch(cna_ctx* ctx, double* G_out);
/* cna_gram_fetch, then the leading kmax eigenpairs of G on the host (cna_host_top_eig: svd_nam's np.linalg.svd, _nam.py:105,
 * as the global test consumes it) and, when they pass the acceptance rule -- residual <= resid_tol * lambda_1,
 * orthogonality <= resid_tol, every leading gap > gap_tol * lambda_1 -- cna_global_test_launch(U, kmax, ks, K, r)
 * (_association.py:35-61,84) in the same call: *accepted = 1, collect with cna_global_test_fetch.  *accepted = 0: G_out
 * is valid, nothing was queued, the caller takes the eigenvectors elsewhere (LAPACK).  use_native = 0: fetch only. */
int  cna_gram_pcs_tests(cna_ctx* ctx, int kmax, const int32_t* ks, int K, int r, int use_native, double resid_tol,
                        double gap_tol, double* G_out /* n_cols x n_cols */, double* U_out /* n_cols x kmax */, int* accepted);
/* out = X . W  (V = NAM^T U / sqrt(svs), _nam.py:106; W = U/sqrt(svs), n_cols x n_w row-major),
 * local rows, row-major n_x_local x n_w */
int  cna_project(cna_ctx* ctx, const double* W, int n_w, double* out_local);
/* cna_project with the result left on the device: read it with cna_fetch_rows(CNA_MAT_PROJ, ...) */
int  cna_project_keep(cna_ctx* ctx, const double* W, int n_w);

/* ---- association (_association.py:77-120, _stats.py:34-83) ----------------------------- */
/* *yes = 1 when the working matrix X on the device is the standardised NAM of the resident walk with every cell and
 * every sample kept and nothing regressed out (what cna_select_standardized leaves for a call without covariates and
 * batches, _nam.py:122,159): it depends on the NAM only, not on the phenotype, so a further analysis of the same dataset
 * keeps it and takes its coefficients with cna_ncorrs (_association.py:77) instead of repeating the selection pass. */
int  cna_x_identity(cna_ctx* ctx, int* yes);
/* ncorrs = (y[:,None]*NAMresid).mean(axis=0) (_association.py:77); kept on the device and
 * optionally copied out (local rows); max_abs = max|ncorrs| over all ranks (_association.py:101). */
int  cna_ncorrs(cna_ctx* ctx, const double* y, double* out_local, double* max_abs);
/* Local null: for P' permuted, conditioned, standardised phenotypes Yc (n_cols x P row-major,
 * _association.py:96-97) count, per permutation p and threshold t,
 *   tails[p][t] = #{cells i : (|X_i . Yc_p| / n_cols)^2 >= edges[t]}
 * = tail_counts(thresholds, nullncorrs) of _stats.py:34-62 with
 * edges[t] = thr_t^2 - 1e-8 - 1e-5*thr_t^2 (ascending).  The cells x P' matrix of
 * _association.py:99 is never materialised.  tails_out is P x T int64, summed over ranks. */
int  cna_null_local(cna_ctx* ctx, const double* Yc, int P, const double* edges, int T,
                    int64_t* tails_out);
/* ---- the permutation test with the phenotypes resident on the device -------------------
 * cna_condition_phenotypes: M is N x N, Y is N x P row-major (observed phenotype in column 0, the
 * permuted ones after it, _association.py:80-83); computes, per column, zcond = M.z / std(M.z, ddof=1)
 * (_association.py:51-52,96-97) and keeps the result on the device.  Sample space only: it runs on
 * the context's second stream and may be called before the working matrix exists (while the
 * diffusion kernels execute); N must equal the matrix's column count when the tests run.
 * cna_null_local_resident: cna_null_local on columns [col0, col0+P) of that resident matrix;
 * tails_out (P x T) and tail_sums_out (T: sum over permutations, all the FDR needs) may each be NULL.
 * cna_global_test: _reg/_stats/_minp_stats (_association.py:35-61) for every resident column:
 * U is n_cols x kmax row-major (first kmax sample-PCs), ks[K] the PC counts tried, r the number
 * of conditioning columns; out: min over k of the F-test p-value (scipy.stats.f.sf semantics),
 * its r2 and the index of the chosen k (-1 when every p is NaN).  All three are replicated work
 * on every rank (sample space). */
int  cna_condition_phenotypes(cna_ctx* ctx, const double* M, const double* Y, int N, int P);
int  cna_null_local_resident(cna_ctx* ctx, int col0, int P, const double* edges, int T, int64_t* tails_out,
                             int64_t* tail_sums_out);
/* cna_null_local_resident in two halves: queue the pass (returns at once; at most one pending),
 * collect its results later.  Between the two the host may call cna_gram_fetch and cna_global_test,
 * which run beside the local-null kernel on a second stream. */
int  cna_null_local_launch(cna_ctx* ctx, int col0, int P, const double* edges, int T, int want_tails,
                           const double* thr /* or NULL: also queue cna_obs_counts(edges, thr) */);
/* the part of a launch that needs only the thresholds (exact cuts, their upload, the observed
 * counts), for callers that know them before the phenotypes are conditioned; follow it with
 * cna_null_local_launch(ctx, col0, P, NULL, T, want_tails, NULL).  No other entry point that uses the
 * context's main scratch (selection, ncorrs, percell) may run in between. */
int  cna_null_local_prepare(cna_ctx* ctx, int P, const double* edges, int T, int want_tails, const double* thr);
int  cna_null_local_fetch(cna_ctx* ctx, int64_t* tails_out, int64_t* tail_sums_out,
                          int64_t* ranks_out, int64_t* num_detected_out /* both NULL unless thr was given */);
/* Error path of _association.py:84-120 on the caller's side: a pass that was launched (cna_null_local_launch, or the
 * fused selection call) and never fetched because the caller raised in between is waited for and dropped, together
 * with a prepared half; the context is ready for the next analysis.  No-op when nothing is pending. */
int  cna_null_local_discard(cna_ctx* ctx);
/* Diagnostics of the last local-null pass that wanted only the sums over permutations (the
 * analysis): such a pass forms the products on the integer matrix cores (csrc/null_i8.hip: 24-bit
 * fixed point, exact int32 accumulation, outputs within the error bound of a cut recomputed in f64)
 * ; the f64 kernel runs the pass again when the integer one gives up.  used_out: 1 when the integer path ran; rechecked_out: outputs it
 * sent to the f64 recheck; fallback_out: 1 when it gave up (queue overflow) and the f64 kernel did
 * the work.  Waits for the device.  Environment CNA_NULL_F64=1 disables the integer path. */
int  cna_null_local_i8_stats(cna_ctx* ctx, int* used_out, int64_t* rechecked_out, int* fallback_out);
int  cna_global_test(cna_ctx* ctx, const double* U, int kmax, const int32_t* ks, int K, int r,
                     double* minp_out, double* r2_out, int32_t* kidx_out);
/* The same in two halves (launch returns at once; U and ks are copied before it returns). */
int  cna_global_test_launch(cna_ctx* ctx, const double* U, int kmax, const int32_t* ks, int K, int r);
int  cna_global_test_fetch(cna_ctx* ctx, double* minp_out, double* r2_out, int32_t* kidx_out);
/* ranks[t] = #{i : ncorrs_i^2 >= edges[t]} (_stats.py:74) and
 * num_detected[t] = #{i : |ncorrs_i| > thr[t]} (_association.py:108), summed over ranks */
int  cna_obs_counts(cna_ctx* ctx, const double* edges, const double* thr, int T,
                    int64_t* ranks_out, int64_t* num_detected_out);
/* data.obs[key] and data.obs[key+'_fdr'] (_association.py:230-237) for ALL n_global cells:
 * coef = NaN for cells not kept else ncorrs; fdr = min{fdr_t : thr_t <= |coef|} else 1.
 * runmin_fdr[t] = min(fdr[0..t]).  kept rows are the ones given to cna_select. */
int  cna_percell_fdr(cna_ctx* ctx, const double* thr, const double* runmin_fdr, int T,
                     double* coef_out_global, double* fdr_out_global);
/* same, into pinned host buffers owned by the context (n_global doubles each; valid until the next
 * call on this context): the D2H copies run at PCIe speed and the caller copies or consumes them */
int  cna_percell_fdr_pinned(cna_ctx* ctx, const double* thr, const double* runmin_fdr, int T,
                            double** coef_ptr, double** fdr_ptr);
/* The coefficient column alone, early: it depends on the observed phenotype only (not on the null),
 * so after cna_ncorrs / cna_select_standardized(y) the caller may queue it ahead of the local-null
 * kernel (launch: returns at once; the copy runs on the second stream under that kernel) and
 * collect the pinned pointer with _wait -- from any thread.  A later cna_percell_fdr_pinned then
 * delivers the FDR column only and returns the same coefficient pointer.  Single rank or local view. */
int  cna_percell_coef_launch(cna_ctx* ctx);
int  cna_percell_coef_wait(cna_ctx* ctx, double** coef_ptr);
/* The FDR column of a pending local-null pass (cna_null_local_launch after cna_percell_coef_launch: the column
 * follows the pass on the device) copied into dst[n] -- the storage of data.obs[key + '_fdr'],
 * _association.py:236-237 -- as soon as it has reached the pinned block: callable from a helper thread while
 * the main thread is inside the samples x samples SVD.  *done = 0: not applicable, nothing copied.
 * cna_percell_fdr_copied_early: *yes = 1 when the column cna_percell_fdr_pinned last returned is that copy. */
int  cna_percell_fdr_copy_early(cna_ctx* ctx, double* dst, int64_t n, int nthreads, int* done);
int  cna_percell_fdr_copied_early(cna_ctx* ctx, int* yes);

/* ---- the fixed-shape analysis in two library calls (round 6) ----------------------------------------------------------
 * cna.tl.association (_association.py:193-242) is ONE straight-line function; for the call shape that needs no decision
 * of the host between its stages -- nsteps given, one batch, covariates allowed, a seed, the local test on -- the stages
 * are queued here without the interpreter in between.  The caller validates the sample-level inputs (check_inputs,
 * _association.py:131-173), uploads graph and sample codes as usual (cna_graph_upload, cna_colsums, cna_set_samples /
 * cna_restart_nam), starts the permutation draw (cna_host_draw_start) and then calls
 *
 *   cna_assoc_begin   the walk of _nam.py:57-70 with a fixed step count: cna_nam_select_hint(y_hint) when given, then
 *                     cna_nam_steps(nsteps); nsteps = 0 keeps the NAM the device holds (the caller's NAM cache).
 *                     Returns once the kernels are queued: the caller builds the projector of _nam.py:128-135 and the
 *                     storage of the two data.obs columns meanwhile.
 *   cna_assoc_finish  compute_nam_and_reindex's selection (_association.py:175-191) + _resid_nam (_nam.py:118-177, no
 *                     batches) as cna_select_standardized_fused; the Gram matrix, its leading eigenpairs and the global
 *                     F-tests (_nam.py:105, _association.py:35-88) as cna_gram_pcs_tests + cna_global_test_fetch; the
 *                     conditioned phenotypes (cna_host_draw_then_condition, or cna_condition_phenotypes once the draw is
 *                     there); the local null (_association.py:91-120) as cna_null_local_launch / _fetch; the FDR table
 *                     (_stats.py:79-80, _association.py:105-108); and the two per-cell columns (_association.py:230-237),
 *                     copied into the caller's storage (coef_dst / fdr_dst) as they arrive.  Blocks until all of it is
 *                     done.  Every stage is the entry point named, in the order the Python host issues them: same bits.
 *
 * status (cna_assoc_out): CNA_ASSOC_DONE; CNA_ASSOC_GENERAL -- a selected cell has zero variance, max|ncorrs| is not
 * finite or the thresholds are out of range: nothing beyond the selection pass was issued, coef_dst / fdr_dst hold
 * nothing, the caller takes its general path (which reports what the reference reports); CNA_ASSOC_NEED_PCS -- the
 * library's eigen-solver stepped aside (cna_gram_pcs_tests: *accepted = 0): everything but the global test is done, G is
 * valid, the caller supplies eigenvectors (LAPACK) through cna_global_test_launch / _fetch; CNA_ASSOC_STALE -- an input
 * listed in `verify_*` no longer hashes to what the device copy was made from: as CNA_ASSOC_GENERAL, after a fresh upload.
 * cna_assoc_run = cna_assoc_begin + cna_assoc_finish for callers with nothing to do in between. */
#define CNA_ASSOC_DONE      0
#define CNA_ASSOC_GENERAL   1
#define CNA_ASSOC_NEED_PCS  2
#define CNA_ASSOC_STALE     3
#define CNA_ASSOC_MAXT      512
typedef struct cna_assoc_args {
  const int32_t* colmap;     /* NAM column of every analysed sample (NAM.reindex(y.index)[filter], _association.py:178-181); NULL: all, in place */
  int32_t n_sel;             /* analysed samples N */
  int32_t r;                 /* conditioning columns (covariates): M = I - C.W, _nam.py:128-135; 0: M = I */
  const double* y;           /* standardised phenotype (numpy ddof=0, _association.py:22), N */
  const double* M;           /* projector, N x N row-major */
  const double* resid_C;     /* N x r standardised covariates (NULL when r = 0) */
  const double* resid_W;     /* r x N: (C^T C)^-1 C^T */
  const int32_t* ks;         /* PC counts of the global test (_association.py:25-28) */
  int32_t K;
  int32_t Nnull;
  const double* table;       /* N x (Nnull + 1) row-major: [y | permuted phenotypes] (_association.py:80-83) */
  int32_t draw_pending;      /* 1: cna_host_draw_start is still filling `table` (this call joins it, the caller collects it) */
  int32_t conditioned;       /* 1: cna_condition_phenotypes(M, table, N, Nnull + 1) has already returned */
  int32_t use_native_eig;    /* cna_gram_pcs_tests' arguments */
  int32_t coef_first;        /* (unused since the eigenpairs run on a thread of their own: the coefficient column never waits for them) */
  double resid_tol, gap_tol;
  double* coef_dst;          /* storage of data.obs[key] / data.obs[key + '_fdr'] (n_dst doubles each), or NULL: */
  double* fdr_dst;           /*   pinned pointers are returned in cna_assoc_out instead */
  int64_t n_dst;
  int32_t copy_threads;
  int32_t n_verify;          /* content checks of the inputs the device copy was made from (the reference re-reads the graph and
                                the ids on every call, _nam.py:25-28,51): cna_host_hash64 of verify_ptr[i] (verify_bytes[i] bytes)
                                must equal verify_hash[i]; taken on a thread of this call while the device works.  A mismatch:
                                status CNA_ASSOC_STALE, nothing is written to coef_dst / fdr_dst */
  const void* verify_ptr[4];
  int64_t verify_bytes[4];
  uint64_t verify_hash[4];
  int32_t verify_threads;
  int32_t reserved;
  double* G;                 /* out: N x N Gram matrix */
  double* U;                 /* out: N x max(ks) leading eigenvectors (valid when eig_accepted) */
  double* minp;              /* out: Nnull + 1 (column 0: the observed phenotype) */
  double* r2;
  int32_t* kidx;
} cna_assoc_args;
typedef struct cna_assoc_out {
  int32_t status, T, eig_accepted, null_fused;
  int32_t coef_in_dst, fdr_in_dst;
  int64_t n_zero;
  double max_abs;
  double* coef_ptr;          /* pinned, valid until the next per-cell call on the context (when not copied to coef_dst) */
  double* fdr_ptr;
  double t_ms[16];           /* when the stages of this call were reached, ms from its entry: [0] phenotypes posted, [1] selection
                                pass back (the walk is over), [2] local null queued, [3] inputs verified, [4] coefficient column
                                out, [5] local null over + FDR column out, [6] null results, [7] eigenpairs + F-tests joined,
                                [8] exit; on the eigenpairs thread: [9] Gram matrix on the host, [10] eigenpairs done and F-tests queued, [11] F-tests fetched; on the draw thread (negative: before this call was entered): [12] permutations drawn,
                                [13] phenotypes conditioned (the flag the fused selection call reads) */
  double thr[CNA_ASSOC_MAXT], fdr[CNA_ASSOC_MAXT], runmin[CNA_ASSOC_MAXT];
  int64_t tail_sums[CNA_ASSOC_MAXT], ranks[CNA_ASSOC_MAXT], num_detected[CNA_ASSOC_MAXT];
} cna_assoc_out;
int  cna_assoc_begin(cna_ctx* ctx, int nsteps, const double* y_hint, int n_hint);
/* the same walk in parts: steps first .. first + count - 1 (0-based) of `total`; y_hint applies to the part that holds the last
 * step.  A caller queues the steps that need only graph and sample codes before it has validated the phenotype. */
int  cna_assoc_begin_part(cna_ctx* ctx, int first, int count, int total, const double* y_hint, int n_hint);
int  cna_assoc_finish(cna_ctx* ctx, const cna_assoc_args* args, cna_assoc_out* out);
int  cna_assoc_run(cna_ctx* ctx, int nsteps, const double* y_hint, int n_hint, const cna_assoc_args* args, cna_assoc_out* out);
/* blocks until the request of cna_host_draw_start (and its follow-up) is done WITHOUT collecting it: the caller's
 * cna_host_draw_wait still returns its status (0 / -1 as cna_host_draw_wait; -2: nothing was started) */
int  cna_host_draw_join(void);
/* out2 = {when the last draw finished, when its follow-up (the conditioning) did}, CLOCK_MONOTONIC seconds: diagnostics */
void cna_host_draw_times(double* out2);

/* ---- device -> host for the lazily materialised result fields (a20) -------------------- */
int  cna_matrix_shape(cna_ctx* ctx, int which, int64_t* n_rows_local, int* n_cols);
/* transposed!=0 writes samples x cells (the reference's orientation), else cells x samples */
int  cna_fetch_matrix(cna_ctx* ctx, int which, double* out, int transposed);
/* FOR TESTS.  The analysis never calls this.  The NAM's rows are ld = round_up(N, 4) doubles apart on the device; every
 * walk step writes zeros into the padding columns N <= col < ld of the rows it stores, and no other fetch reaches them.
 * *n_pad_cols = ld - N; out (n_local x n_pad_cols, may be NULL to ask for the count alone) receives those columns of
 * every local row of the NAM, in device cell order.  The NAM only: the padding of the walk's state buffers, which the
 * step kernels write the same way, is not read back.  CNA_ESTATE without a NAM. */
int  cna_fetch_nam_padding(cna_ctx* ctx, double* out, int* n_pad_cols);
/* the same with rows and columns picked and ordered on the device: out[i][j] = M[rows[i]][cols[j]]
 * (n_out x n_cols, or its transpose); rows / cols NULL = all, in order.  rows are local row indices
 * of the matrix.  One gather kernel + one contiguous copy: the caller's cell order and orientation
 * (res.nam, res.namresid, cna.tl.nam: _nam.py:73,193) cost no cells x samples reshuffle on the host. */
int  cna_fetch_rows(cna_ctx* ctx, int which, const int64_t* rows, int64_t n_out,
                    const int32_t* cols, int n_cols, double* out, int transposed);

/* concatenate count_local doubles from every rank, in rank order, into out_all on every rank
 * (row blocks of the lazily fetched matrices when the job spans several GPUs) */
int  cna_allgather_host(cna_ctx* ctx, const double* local, int64_t count_local, double* out_all,
                        int64_t count_total);

/* ---- host-side helper: the permutation draw's random stream (_stats.py:10) ----------------- */
/* n values of np.random.randn from numpy's legacy generator, bit for bit, vectorised (host code
 * only, no device involved; csrc/host_rng.c).  key[624] / *pos / *has_gauss / *gauss: the state as
 * np.random.get_state() reports it, advanced in place to where numpy's own draw would leave it.
 * No context: callable from any thread. */
int  cna_host_legacy_randn(uint32_t* key, int* pos, int* has_gauss, double* gauss, int64_t n, double* out);
/* threads the two host helpers of csrc/host_rng.c may use for LARGE draws (default 1; results do not depend on it) */
void cna_host_set_threads(int n);
/* out[rows[i]][c] = y[argsort(R[:, c])[i]] for the m x num draws R (row-major): the permuted phenotypes of
 * conditional_permutation / grouplevel_permutation (_stats.py:11-17,31) for large draws, columns split over
 * threads (host only; rows NULL = identity) */
int  cna_host_argsort_gather(const double* R, int m, int num, const double* y, double* out, int64_t ld_out,
                             const int64_t* rows);
/* The whole draw of conditional_permutation (reference _stats.py:4-18: per level of the batch vector, in np.unique
 * order, Y[members][argsort(randn(len(members), num), axis=0)]) on the library's own host thread, so that it runs
 * beside the caller's interpreter instead of inside it.  key / pos: numpy's MT19937 state memory, freshly seeded (no
 * cached normal), num even; members[lev_off[l] .. lev_off[l+1]) = rows of level l; out[r * ld_out + p] receives the
 * permuted phenotypes.  All pointers stay valid until cna_host_draw_wait() has returned (0; -1: the draw failed and the
 * generator state is undefined; -2: nothing started).  cna_host_draw_start: 0 = accepted, -1 = not accepted, nothing
 * touched.  One request at a time per process. */
int  cna_host_draw_start(uint32_t* key, int* pos, const double* y, int m, int num, int nlev, const int64_t* lev_off,
                         const int64_t* members, double* out, int64_t ld_out, int threads);
/* cna_host_draw_start that also records WHICH row of y every output was taken from (idx_out: m x num int32 row-major): the
 * permutations of a seeded draw depend on (seed, m, num, levels) only -- not on y -- so a caller that tests many phenotypes
 * with one seed (the demo does: demo/demo.ipynb:156,251) replays them with cna_host_gather_rows, out[r][p] = y[idx[r][p]]
 * (= Y[bix], _stats.py:16-17), instead of drawing and sorting again; numpy's generator is then put where the recorded draw
 * left it (the caller keeps that state next to idx). */
int  cna_host_draw_start_idx(uint32_t* key, int* pos, const double* y, int m, int num, int nlev, const int64_t* lev_off,
                             const int64_t* members, double* out, int64_t ld_out, int threads, int32_t* idx_out);
int  cna_host_gather_rows(const double* y, const int32_t* idx, int m, int num, double* out, int64_t ld_out, int nthreads);
/* follow-up of the request under way: the worker conditions the phenotypes itself when the draw is there --
 * cna_condition_phenotypes(ctx, M, table, N, cols) with table = the N x cols matrix [y | permutations] being filled --
 * and stores 1 / -1 (failed) in *flag.  0 accepted, -1 nothing to follow.  cna_host_draw_wait covers it. */
int  cna_host_draw_then_condition(cna_ctx* ctx, const double* M, const double* table, int N, int cols, int* flag);
int  cna_host_draw_wait(void);

/* ---- host-side helpers: graph identity and the device cell order (csrc/host_graph.c) ------- */
/* 64-bit content hash of a buffer, computed on up to nthreads threads (the value does not depend on the
 * thread count).  The engine keys the resident graph on the hash of ALL of data / indices / indptr, so an
 * in-place edit of any entry re-uploads the graph -- the reference reads `data.obsp['connectivities']`
 * afresh on every call (_nam.py:25-28). */
uint64_t cna_host_hash64(const void* p, int64_t nbytes, int nthreads);
/* memcpy on up to nthreads threads (the per-cell result columns into the caller's frame,
 * _association.py:230-237 of the reference assigns them to data.obs) */
int  cna_host_copy(void* dst, const void* src, int64_t nbytes, int nthreads);
/* dst[i] = bins[i] > 0 ? runmin[bins[i] - 1] : 1.0 on nthreads threads: the per-cell FDR column (_association.py:234-237)
 * from the per-cell threshold counts #{t : thr_t <= |coef_i|} and the running minimum of the FDR table */
int  cna_host_expand_u16(double* dst, const uint16_t* bins, int64_t n, const double* runmin, int T, int nthreads);
/* Device cell order: clusters of B cells grown greedily by "most edges into the cluster" so that the
 * rows of one block share neighbours (edges / distinct neighbour rows of a block: 3.0 at B = 64 against
 * 2.0 for reverse Cuthill-McKee).  indptr int64[n+1], indices int32 of the rows' columns (columns outside
 * [0, n) are ignored); order_out[i] = caller's index of device row i.  Returns the number of cells placed
 * in full clusters, -1 when out of memory.  Only the numbering changes: every row keeps its neighbours in
 * the caller's CSR order, so no sum is reordered (_nam.py:33). */
int64_t cna_host_cluster_order(int64_t n, const int64_t* indptr, const int32_t* indices, int B, int64_t* order_out);
/* The same on several threads: the cells are first split into n / 65536 (<= 64) connected regions by a multi-source
 * breadth-first search, every region is ordered as above on its own (in parallel), full clusters of all regions first.
 * The result depends on n and the graph only, not on nthreads.  Below 131072 cells: the sequential order. */
int64_t cna_host_cluster_order_mt(int64_t n, const int64_t* indptr, const int32_t* indices, int B, int nthreads,
                                  int64_t* order_out);
/* graph of the clusters of a cell order (cluster c = order[c * B .. (c + 1) * B)): per cluster the clusters its cells
 * have edges into and how many; first call with col == NULL fills ptr[nc + 1] and returns the entry count, the second
 * fills col / cnt.  Host only; the blocks of a sharded run are packed from it (cna_amd._order.partition_order). */
int64_t cna_host_cluster_graph(int64_t n, const int64_t* indptr, const int32_t* indices, const int64_t* order, int B,
                               int64_t* ptr, int32_t* col, int64_t* cnt);
/* Rows [r0, r1) of the graph in the device order: out row i = caller's row perm[r0 + i], columns relabelled
 * through col_map and left in their original order; values (vbytes = 4 | 8) copied bit for bit.  Sizes from
 * cna_host_permuted_nnz.  Threaded; integer work only. */
int64_t cna_host_permuted_nnz(const int64_t* perm, int64_t r0, int64_t r1, const int64_t* indptr);
int  cna_host_permute_rows(const int64_t* perm, int64_t r0, int64_t r1, const int64_t* indptr, const int32_t* indices,
                           const void* data, int vbytes, const int64_t* col_map, int64_t* out_indptr,
                           int32_t* out_indices, void* out_data, int nthreads);

/* ---- benchmark / test input: kNN connectivities graph built on the device (csrc/knn.hip) ---- */
/* Stand-in for scanpy.pp.neighbors (demo/demo.ipynb:590, makedata.ipynb:117) on synthetic points: exact
 * brute-force kNN of X (n x d float32, d <= 64; k counts the point itself, 2 <= k <= 65), UMAP smooth-kNN
 * weights, fuzzy union A + A^T - A o A^T; CSR with sorted int32 column indices, float32 values, empty
 * diagonal.  indices_out / data_out: room for 2 n (k-1) entries.  An input generator, not a parity target. */
int  cna_knn_graph(cna_ctx* ctx, const float* X, int64_t n, int d, int k, int64_t* indptr_out,
                   int32_t* indices_out, float* data_out, int64_t* nnz_out);

/* ---- per-gene correlation to per-cell columns (csrc/genes.hip, expr_corr.hip) ----------------- */
/* The step of the reference's workflow that follows cna.tl.association (demo/demo.ipynb, "per-gene correlations to
 * neighborhood coefficient"):
 *     d.var['corr_case'] = np.corrcoef(d.obs.male_coef.values.reshape(1,-1), d.X, rowvar=False)[0,1:]
 * with the expression matrix d.X resident on the device.  One matrix per context, in the CALLER's cell order; it is
 * derived from nothing else the context holds (graph, walk, NAM, working matrix, device cell order) and nothing else is
 * derived from it, so these entry points may be called at any point of an analysis -- also between the launch and the
 * fetch of a local-null pass -- and work on a context that never saw a graph.  They use a stream of their own. */

/* d.X of that line as a C-contiguous n_cells x n_genes array, float32 or float64 (demo/demo.ipynb, "per-gene
 * correlations to neighborhood coefficient").  Replaces the resident matrix, if any.  1 <= n_cells, n_genes < 2^31.
 * CNA_ENOMEM: it does not fit; the context then holds no expression matrix. */
int  cna_expr_upload_dense(cna_ctx* ctx, const void* x, int64_t n_cells, int64_t n_genes, int is_f64);
/* The same d.X as a scipy CSR (is_csc = 0: indptr has n_cells + 1 entries, indices are genes) or CSC (is_csc = 1:
 * n_genes + 1 entries, indices are cells) matrix, which np.corrcoef of that line (demo/demo.ipynb, "per-gene
 * correlations to neighborhood coefficient") cannot take at all.  index_bytes: 4 or 8, for indptr and indices alike;
 * values float32 or float64; nnz < 2^63.  Canonical form is expected (indices ascending inside a row / column, no
 * duplicates -- what scipy's sum_duplicates() leaves; explicit zeros may stay).  The device keeps gene-major lists
 * {cell, value}, cells ascending: a CSC upload is that already, a CSR upload is transposed on the device by counting
 * (stable in the cell index, so both give the same lists and the same bits later).  The transpose needs the rows'
 * indices and values beside the result for a moment: CNA_ENOMEM, with nothing resident afterwards, when that does
 * not fit.  CNA_EINVAL: offsets that do not start at 0 / fall / end elsewhere than nnz, or an index out of range. */
int  cna_expr_upload_sparse(cna_ctx* ctx, const void* indptr, const void* indices, const void* data, int64_t n_cells,
                            int64_t n_genes, int64_t nnz, int index_bytes, int is_f64, int is_csc);
/* Forget the resident d.X of that line (demo/demo.ipynb, "per-gene correlations to neighborhood coefficient") and the
 * work buffers of cna_gene_corr, cna_expr_to_bins, cna_expr_cross, cna_coef_strata, cna_gene_corr_by, cna_matrix_to_bins,
 * cna_enrichment_extremes, cna_expr_cross_by, cna_gram_by, cna_coef_raster, cna_graph_components_find,
 * cna_gene_ranksum_by, cna_gene_ranksum_pairs, cna_gene_ranksum_within, cna_gene_rank_corr, cna_gene_rank_corr_by,
 * cna_nbhd_expr and cna_gene_nbhd_corr: cna_ctx_device_bytes returns to what it was before the upload. */
int  cna_expr_drop(cna_ctx* ctx);
/* What is resident: *format 0 nothing, 1 the dense array, 2 gene-major lists; *n_uploads counts the uploads this context
 * has performed so far (it survives cna_expr_drop: callers check residency with it).  Any pointer may be NULL. */
int  cna_expr_shape(cna_ctx* ctx, int64_t* n_cells, int64_t* n_genes, int64_t* nnz, int* format, int* is_f64,
                    int64_t* n_uploads);
/* r_out[j * n_genes + g] = Pearson correlation of gene g of the resident matrix with column j of V (q x n_cells
 * row-major, caller's cell order, 1 <= q <= 16) over the cells where V[j] is finite -- each column has its own such
 * set; NaN marks the cells cna.tl.association did not keep.  With every cell finite this is row 0 of
 * np.corrcoef(v, X, rowvar=False) without its first entry (demo/demo.ipynb, "per-gene correlations to
 * neighborhood coefficient"), computed in one pass over X instead of a (genes + 1)^2 matrix: per gene the sums of x,
 * x^2 and x (v - mean v), float64, in a fixed order (no floating-point atomics: the same bits on every run).  NaN
 * where numpy's 0 / 0 gives NaN: a gene that is constant over the column's cells, decided exactly (minimum ==
 * maximum), a constant column, fewer than two finite cells; NaN / inf inside X reach that gene's result.
 * CNA_ESTATE: no expression matrix is resident. */
int  cna_gene_corr(cna_ctx* ctx, const double* V, int q, double* r_out);

/* ---- per-bin sums of the resident expression matrix (csrc/expr_bins.hip) --------------------- */
/* The sample-level side of the reference's workflow: utils/multisample.py:4-11 (obs_to_sample) turns per-cell columns of
 * d.obs into one row per sample; this is the same aggregation for d.X, the samples x genes matrix of summed expression
 * ("pseudobulk"), over the matrix cna_expr_upload_* left on the device, dense or gene-major.  codes[i] is the bin (row of
 * the result) of cell i in the CALLER's cell order, -1 for a cell that is left out; 1 <= n_bins <= 4096.
 *   what = 0: sums_out[b * n_genes + g] = sum of x[i, g] over the cells of bin b
 *   what = 1: ... = number of those cells with x[i, g] > 0 (an explicit zero of a sparse upload does not count)
 * counts_out[b] = cells of bin b.  The means and fractions of cna.ut.expr_to_sample are these over counts_out, divided
 * by the caller in float64: the device returns sums and integers only.  Sums are float64 in a fixed order (the cells of a
 * bin ascending, cut into chunks whose partials are added in chunk order; no floating-point atomics): two runs give the
 * same bits, and so do a CSR and a CSC upload of one matrix.  A bin without cells gives 0; NaN / inf inside X reach
 * their own (bin, gene) only.
 * Like cna_gene_corr it runs on the expression stream with buffers of its own (grow-only, freed by cna_expr_drop), works on
 * a context that never saw a graph, and may be called between cna_null_local_launch and cna_null_local_fetch.
 * CNA_ESTATE: no expression matrix is resident.  CNA_EINVAL: n_bins or what out of range, or a code outside
 * [-1, n_bins) -- found on the device before any sum is formed; nothing is written then. */
int  cna_expr_to_bins(cna_ctx* ctx, const int32_t* codes, int n_bins, int what, double* sums_out, int64_t* counts_out);

/* ---- the neighbourhood coefficient by cluster (csrc/strata.hip) ------------------------------ */
/* The step of the reference's workflow between cna.tl.association and the per-gene correlations (demo/demo.ipynb):
 *     sc.tl.leiden(d); cna.pl.violinplot(d, 'leiden', key='coef')
 * (plotting/_strat.py:21-29 hands data.obs[key] of every level to Axes.violinplot, i.e. to matplotlib.cbook.violin_stats
 * with mlab.GaussianKDE) as numbers: per bin the counts, the moments, the exact median and the kernel density on the grid
 * that gets drawn, plus the cells that pass the FDR with either sign (plotting/_umap.py:10).
 *   v[i]      the coefficient of cell i (CALLER's cell order; NaN / inf = the cell has none), n_cells in [1, 2^31)
 *   fdr[i]    its FDR, or fdr = NULL (n_pos_out / n_neg_out are then 0)
 *   codes[i]  its bin, -1 for a cell that is left out; 1 <= n_bins <= 1024
 * A cell is KEPT when its code is >= 0 and v[i] is finite.  Per bin b:
 *   n_out = cells with that code, n_kept_out = kept cells, n_pos_out / n_neg_out = kept cells with fdr[i] <= fdr_thresh (a
 *   NaN fdr fails) and v > 0 / v < 0; mean_out, ssd_out = sum (v - mean)^2 (two passes), min_out, median_out (np.median:
 *   both middle order statistics by an exact radix select, (a + b) / 2), max_out over the kept cells -- NaN for a bin that
 *   keeps none (ssd 0 for one that keeps one).
 *   vals_out[b * points + j], 1 <= points <= 1024: the density at x_j = min + j * step, step = (max - min) / (points - 1),
 *   the last point max itself (np.linspace(min, max, points), which the caller forms from min_out / max_out).  All kept values
 *   equal (min == max, decided exactly; this includes a single one): Axes.violinplot's fallback (x_j == value) = 1.
 *   Otherwise mlab.GaussianKDE in its own order: var = ssd / (m - 1), f the bandwidth factor, inv = (1 / var) / f^2,
 *   vals = sum_i exp(-(d * (inv * d)) / 2) / (sqrt(2 pi var f^2) * m), d = v_i - x_j; bw_kind 0: f = m^-0.2 (Scott),
 *   1: f = (3 m / 4)^-0.2 (Silverman), 2: f = bw_value > 0.  A bin that keeps no cell gives 0.  float64 exp throughout.
 * Sums are float64 in a fixed order (the kept values of a bin in cell order, cut into chunks whose partials are added in
 * chunk order; no floating-point atomics): two runs give the same bits.
 * Like the expression entry points it depends on nothing else the context holds and nothing depends on it: no graph and no
 * resident expression matrix are needed, and it may be called between cna_null_local_launch and cna_null_local_fetch.  It
 * runs on the expression stream with grow-only buffers of its own, freed by cna_expr_drop (and with the context).
 * CNA_EINVAL, with nothing written: a parameter out of range, or a code outside [-1, n_bins) -- found on the device before
 * any sum is formed. */
int  cna_coef_strata(cna_ctx* ctx, const double* v, const double* fdr, const int32_t* codes, int64_t n_cells, int n_bins,
                     int points, int bw_kind, double bw_value, double fdr_thresh, int64_t* n_out, int64_t* n_kept_out,
                     int64_t* n_pos_out, int64_t* n_neg_out, double* mean_out, double* ssd_out, double* min_out,
                     double* median_out, double* max_out, double* vals_out);

/* ---- per-gene correlations inside every level of a clustering (csrc/expr_corr_by.hip) -------- */
/* The question after cna.pl.violinplot(d, 'leiden', key='coef') (plotting/_strat.py:21-29) shows a cluster whose violin
 * spans both signs: which genes separate its expanded cells from its depleted ones?  The global line of demo/demo.ipynb
 * ("per-gene correlations to neighborhood coefficient") cannot say, it is dominated by the cluster markers.  One pass over
 * the resident matrix, the cell's level as the accumulator index:
 *   V         q x n_cells row-major, 1 <= q <= 16, CALLER's cell order; a non-finite value leaves the cell out of that key
 *   codes[i]  the level of cell i, -1 for a cell that is left out; 1 <= n_bins <= 1024 and q x n_bins <= 4096
 * For key j and level L let C = the cells with code L and a finite V[j]:
 *   n_out[j * n_bins + L] = |C|
 *   r_out[(j * n_bins + L) * n_genes + g] = Pearson correlation of gene g with V[j] over C (implicit zeros of a sparse upload
 *   count), by the rules of cna_gene_corr level by level: the key is centred on its mean over C before it is multiplied; NaN
 *   where |C| < 2, where V[j] is constant on C or the gene is (minimum == maximum, decided exactly); otherwise clipped to
 *   [-1, 1].
 *   within_out[j * n_genes + g] (may be NULL) = the pooled within-level correlation, sum_L cov_L / sqrt(sum_L varx_L *
 *   sum_L varv_L) with the centred sums of every level: the correlation of (x - level mean) with (v - level mean) over the
 *   cells that have a level and a finite V[j].  A level where the gene is constant adds exactly 0 to cov and varx, one where
 *   the key is constant exactly 0 to cov and varv; NaN when no level has the gene, or none the key, non-constant.
 * Sums are float64 in a fixed order (the cells of a level ascending, cut into chunks whose partials are added in chunk order,
 * the levels ascending; no floating-point atomics): two runs give the same bits.  Runs on the expression stream with
 * grow-only buffers of its own (freed by cna_expr_drop) and changes no other state.
 * CNA_ESTATE: no expression matrix is resident.  CNA_EINVAL, with nothing written: q or n_bins out of range, or a code
 * outside [-1, n_bins) -- found on the device before any sum is formed. */
int  cna_gene_corr_by(cna_ctx* ctx, const double* V, int q, const int32_t* codes, int n_bins, double* r_out,
                      double* within_out, int64_t* n_out);

/* ---- exact rank sums of every level against the rest, per gene (csrc/expr_ranksum.hip) -------- */
/* The question after cna.tl.coef_populations (or sc.tl.leiden) has named groups of cells: which genes mark each group
 * against all other cells?  The statistic is the Wilcoxon rank sum / Mann-Whitney U of scanpy's
 * rank_genes_groups(method='wilcoxon'); it needs a ranking of the CELLS of every gene, and one ranking over all kept
 * cells serves every level: the level's rank sum is the sum of those ranks over its cells.
 *   codes[i]  the level of cell i (CALLER's cell order), -1 for a cell that is left out; 1 <= n_bins <= 1024
 *   work_bytes  what the keys, the levels and their ping-pong copies of one tile of whole genes may take; 0: 1 GiB.  A
 *             gene that alone exceeds it is one tile.  The sort's counters (1 KB per chunk of a gene's list) come on top
 * The m kept cells are those with a code >= 0.  Per gene g the kept cells are ranked by x[i,g] with midranks: less(i)
 * and lesseq(i) count the kept cells with a smaller / a not larger value.
 *   rank2_out[b * n_genes + g] = sum over the cells of level b of less + lesseq + 1: twice the rank sum, <= m (m + 1)
 *   tie_out[g] = sum over the tie groups of t^3 - t, each term (double)t * (double)(t * t - 1) with t * t - 1 in 64-bit
 *   integers, added in a fixed order: exact whenever the total is below 2^53, the same bits on every run and for a CSR
 *   and a CSC upload of one matrix
 *   n_out[b] = cells of level b
 *   nan_out[g] = 1 when a KEPT cell holds NaN in gene g (the gene's other outputs are then unspecified); a NaN in a
 *   left-out cell sets nothing
 * Order is by value: +-inf are ordinary values, -0.0 equals +0.0, a stored zero of a sparse upload equals the implicit
 * ones, and a float64 matrix is ranked on all 64 bits (two values that round to one float32 are no tie).
 * A stable LSD radix sort segmented by gene (8 bits per pass: 4 passes for float32, 8 for float64) orders {key, level};
 * on the gene-major form only the stored entries are sorted, the implicit zeros are one tie group placed by arithmetic.
 * Like its siblings it runs on the expression stream with grow-only buffers of its own (freed by cna_expr_drop), changes
 * no other state, works on a context that never saw a graph and may be called between cna_null_local_launch and
 * cna_null_local_fetch.
 * CNA_ESTATE: no expression matrix is resident.  CNA_EINVAL, with nothing written: n_bins or work_bytes out of range,
 * or a code outside [-1, n_bins) -- found on the device before anything else runs. */
int  cna_gene_ranksum_by(cna_ctx* ctx, const int32_t* codes, int n_bins, int64_t work_bytes, int64_t* rank2_out,
                         double* tie_out, int64_t* n_out, uint8_t* nan_out);
/* Level against level from the same ranking: what separates 'pos1' from 'neg1', or every population from one reference
 * (scanpy's rank_genes_groups(reference=...)).  Order within the union of two levels is the order within all kept cells, so
 * the one sort of cna_gene_ranksum_by gives every pair at once.  Walk the tie groups of a gene in ascending order; with
 * c[l] the kept cells of level l in a group and C[l] those strictly below it,
 *   u2_out[k * n_genes + g]  = sum over the groups of c[a] (2 C[b] + c[b]) = 2 U_ab for pair k = (a, b) = (pairs[2k],
 *   pairs[2k + 1]): twice scipy.stats.mannwhitneyu(x_a, x_b).statistic, an integer; 0 when either level is empty;
 *   u2_ab + u2_ba = 2 n_a n_b
 *   tie_out[k * n_genes + g] = sum over the groups of t^3 - t, t = c[a] + c[b]: the tie term over a u b.  Accumulated in
 *   integers (96 bits per accumulator: enough for 2^31 cells) and rounded to double once at the end: exact whenever
 *   below 2^53, the same bits on every run and for a CSR and a CSC upload of one matrix
 *   n_out[b], nan_out[g]     as in cna_gene_ranksum_by (a NaN in a kept cell of ANY level flags the gene for every pair)
 * codes, work_bytes, the value semantics (-0.0 = +0.0 = a stored zero = the implicit zeros, +-inf ordinary, float64 on 64
 * bits), the keys and the sort are those of cna_gene_ranksum_by; the kept cells are those with a code >= 0.
 *   1 <= n_bins <= 64 levels take part; 1 <= n_pairs <= 2016; every pair has a != b, both in [0, n_bins); a pair may repeat
 *   and (b, a) may stand beside (a, b).
 * Behind the sort one workgroup per gene walks the sorted list forward once, per-level prefix counts from wave ballots and
 * one integer accumulator per unordered pair of levels in LDS; the implicit zeros of the gene-major form join the stored
 * zeros' group by arithmetic.  Runs on the expression stream with the work buffers of cna_gene_ranksum_by (grow-only, freed
 * by cna_expr_drop), changes no other state, works on a context that never saw a graph and may be called between
 * cna_null_local_launch and cna_null_local_fetch.
 * CNA_ESTATE: no expression matrix is resident.  CNA_EINVAL, with nothing written: a null pointer, n_bins, n_pairs or
 * work_bytes out of range, a pair with a == b or a level outside [0, n_bins) (checked on the host), or a code outside
 * [-1, n_bins) -- found on the device before anything else runs.  CNA_ENOMEM: the two n_pairs x n_genes result buffers do
 * not fit; the context stays usable. */
int  cna_gene_ranksum_pairs(cna_ctx* ctx, const int32_t* codes, int n_bins, const int32_t* pairs, int n_pairs,
                            int64_t work_bytes, int64_t* u2_out, double* tie_out, int64_t* n_out, uint8_t* nan_out);
/* Every level against the rest INSIDE every block of a second per-cell column (the sample or the batch), the blocks folded
 * with the caller's weights: the integers and weighted sums of the stratified rank-sum test (van Elteren's test;
 * cna.tl.gene_markers_within).  A population found by an association with a sample-level phenotype is over-represented in
 * some samples by construction, so the pooled ranking of cna_gene_ranksum_by calls a gene a marker whose baseline differs
 * between donors or batches; ranked inside each block such a gene shows nothing.
 *   codes[i]   the level of cell i in [0, n_bins), or -1;   1 <= n_bins <= 1024
 *   blocks[i]  the block of cell i in [0, n_blocks), or -1;  1 <= n_blocks <= 255 (the block is one digit of the sort and
 *              255 stands for a left-out entry, as the level does in cna_gene_rank_corr_by)
 *   w_num[s], w_tie[s * n_bins + l]   finite weights of block s: of its centred rank sums and, per level, of its tie term
 *   work_bytes  as in cna_gene_ranksum_by, for {key, cell} entries: 2 x (4 or 8, + 4) bytes each
 * The KEPT cells are those with a level code >= 0 AND a block code >= 0.  For block s, level l and gene g: n_s the kept
 * cells of the block, n_sl those of level l, R_gsl the sum over the level's cells of their midranks inside the block, T_gs
 * the sum of t^3 - t over the gene's tie groups inside the block, under the value rules of cna_gene_ranksum_by (-0.0 =
 * +0.0 = a stored zero = the implicit zeros, +-inf ordinary values, float64 ranked on all 64 bits).
 * D_gsl = 2 R_gsl - n_sl (n_s + 1) is an integer, twice the centred rank sum: D / 2 = U_gsl - n_sl (n_s - n_sl) / 2.
 *   n_out[s * n_bins + l] = n_sl
 *   d2_out[l * n_genes + g] = sum over s of D_gsl, exact; |sum| <= m^2 for m kept cells
 *   num_out[l * n_genes + g]: acc = +0.0; for s = 0 .. n_blocks - 1 in that order, empty blocks included,
 *             acc = acc + w_num[s] * (double)D_gsl, the product and the sum rounded separately (no FMA contraction): the
 *             bits of that loop in numpy
 *   tiew_out[l * n_genes + g]: the same fold of w_tie[s * n_bins + l] * T_gs, T_gs a double formed like
 *             cna_gene_ranksum_by's tie_out (exact below 2^53)
 *   live_out[l * n_genes + g] = the blocks with 0 < n_sl < n_s in which gene g is not constant, decided from the tie runs
 *             (the zero group holds all n_s cells, or all n_s are stored in one run), not from a floating comparison
 *   nan_out[g] = 1 when a kept cell of ANY block holds NaN in gene g (the gene's other outputs are then unspecified)
 * Behind the value passes of cna_gene_ranksum_by's sort, with the cell as the entry's payload, one more stable pass takes
 * the block of the entry's cell as its digit, which leaves every gene's list block-major and sorted inside a block, the scan
 * of that pass saying where each (gene, block) begins: one sort instead of one per block.  One workgroup per gene then
 * takes the blocks in order: cna_gene_ranksum_by's walk on the block's sub-list with n_s cells, its stored entries and
 * n_s - stored implicit zeros, the level read from codes[cell], per-level integer sums in LDS; behind a block one thread
 * per level folds it into the level's accumulators, which fixes the order of the float adds.
 * The same bits on every run, under every work_bytes and for a CSR and a CSC upload of one matrix.  Runs on the expression
 * stream with the work buffers of cna_gene_ranksum_by (grow-only, freed by cna_expr_drop), changes no other state, works
 * on a context that never saw a graph and may be called between cna_null_local_launch and cna_null_local_fetch.  Its
 * kernel behind the sort is timed under CNA_K_RANKSUM_RANK, the keys, the sort and the copies back under _KEYS, _SORT
 * and _FETCH.
 * CNA_ESTATE: no expression matrix is resident.  CNA_EINVAL, with nothing written: a null pointer, n_bins, n_blocks or
 * work_bytes out of range, a weight that is not finite, a level code outside [-1, n_bins) or a block code outside
 * [-1, n_blocks) (checked on the host, with the table of n_sl).  CNA_ENOMEM: the four n_bins x n_genes result buffers do
 * not fit; the context stays usable. */
int  cna_gene_ranksum_within(cna_ctx* ctx, const int32_t* codes, int n_bins, const int32_t* blocks, int n_blocks,
                             const double* w_num, const double* w_tie, int64_t work_bytes, int64_t* d2_out, double* num_out,
                             double* tiew_out, int32_t* live_out, int64_t* n_out, uint8_t* nan_out);

/* Spearman's rank correlation of every gene with 1 <= q <= 16 per-cell columns (cna.tl.gene_rank_corr), from the same sort
 * with the cell as the entry's payload: invariant to log1p, scaling and every other monotone normalisation of X or of a
 * column, which cna_gene_corr's Pearson r is not.
 *   V[k * n_cells + i]  column k in cell i (CALLER's cell order).  The m KEPT cells are those where EVERY column is finite:
 *             one set per call (a gene's ranks depend on the set), unlike cna_gene_corr's set per column
 *   work_bytes  as in cna_gene_ranksum_by, for {key, cell} entries: 2 x (4 or 8, + 4) bytes each; the columns are sorted
 *             within the same budget, q segments of n_cells entries of 2 x (8 + 4) bytes, one column at least at a time
 * Genes and columns are ranked over the kept cells with midranks: a gene on the stored type's bits by the rules of
 * cna_gene_ranksum_by (-0.0 = +0.0 = a stored zero = the implicit zeros, +-inf ordinary, float64 on 64 bits), a column as
 * float64 on all 64 bits with -0.0 = +0.0.  With r the midrank, a_i = 2 r_gene(i) - (m + 1) and b_i = 2 r_column(i) -
 * (m + 1): integers below m in absolute value that sum to 0 over the kept cells.
 *   s_lo_out[k * n_genes + g], s_hi_out[k * n_genes + g]   S = sum over the kept cells of a_i b_i in 128-bit two's
 *             complement: the low 64 bits and the limb above them.  |S| <= (m^3 - m) / 3, which passes 2^63 from
 *             3 024 617 cells on; nothing is rounded and no m is refused
 *   tie_gene_out[g]   sum over the tie groups of t^3 - t, formed like cna_gene_ranksum_by's tie_out
 *   tie_key_out[k]    the same for column k, summed in integers (96 bits) and rounded to double once: exact below 2^53
 *   *m_out = m;  nan_out[g] as in cna_gene_ranksum_by (the gene's other outputs are then unspecified)
 * so that rho = 3 S / sqrt((m^3 - m - tie_gene) (m^3 - m - tie_key)), scipy.stats.spearmanr's statistic; the float64
 * line is the caller's (cna_amd/tools/_gene_rank_corr.py: rank_corr_statistics), with NaN for a constant gene or column
 * (tie = m^3 - m), m < 2 and a flagged gene.  No p-value: cells are not independent (cna.tl.gene_test).
 * One thread per kept entry of a column finds its tie run [s, e) in the column's sorted segment (a binary search where a
 * neighbour ties) and writes b = s + e - m into a cell-major table; one workgroup per gene walks the gene's sorted list forward for s and backward for e, gathers
 * the cell's row of that table and adds coefficient x b per column in integer registers, folded in a fixed order; the
 * implicit zeros of the gene-major form are one group whose share is -a_0 x (sum of b over the stored kept entries).
 * The same bits on every run, under every work_bytes and for a CSR and a CSC upload of one matrix.
 * Runs on the expression stream with the work buffers of cna_gene_ranksum_by (grow-only, freed by cna_expr_drop), changes
 * no other state, works on a context that never saw a graph and may be called between cna_null_local_launch and
 * cna_null_local_fetch.
 * CNA_ESTATE: no expression matrix is resident.  CNA_EINVAL, with nothing written: a null pointer, q outside [1, 16] or
 * a negative work_bytes. */
int  cna_gene_rank_corr(cna_ctx* ctx, const double* V, int q, int64_t work_bytes, uint64_t* s_lo_out, int64_t* s_hi_out,
                        double* tie_gene_out, double* tie_key_out, int64_t* m_out, uint8_t* nan_out);

/* The same inside every level of a clustering (cna.tl.gene_rank_corr_strata): for level l, column k and gene g the integers
 * of scipy.stats.spearmanr(x_g[C_l], v_k[C_l]), where C_l holds the cells of level l in which EVERY column of the call is
 * finite -- cna_gene_rank_corr's one kept set per call, intersected with the level -- and genes and columns are ranked
 * with midranks over C_l, under cna_gene_rank_corr's rules for ties and zeros.
 *   codes[i]  the level of cell i in [0, n_bins), or -1: the cell is left out.  1 <= n_bins <= 255
 *   s_lo_out, s_hi_out [(l * q + k) * n_genes + g]   S of level l: a and b are 2 x midrank - (m_l + 1), ranked inside C_l
 *   tie_gene_out[l * n_genes + g], tie_key_out[l * q + k]   the tie terms inside C_l, formed as cna_gene_rank_corr's
 *   m_out[l] = m_l = |C_l|
 *   nan_out[g]  a cell of ANY C_l holds NaN in gene g: a guard on the whole gene (its other outputs are unspecified in
 *             every level), not scipy's behaviour level by level
 * so that rho of level l is rank_corr_statistics' line on the level's slices, NaN for a gene that is constant on C_l (a
 * sparse gene with no stored entry there among them), a column that is constant on C_l and m_l < 2.  Level l equals
 * cna_gene_rank_corr called with the columns set to NaN outside level l, integer for integer (s_lo, s_hi, both tie terms
 * and m), from one sort of the matrix instead of one per level: behind the value passes one more stable radix pass takes
 * the level of the entry's cell as its digit (255: a left-out entry), which leaves every gene's list, and every column's
 * segment, level-major and sorted by value inside a level, the scan of that pass being the table of where each (gene,
 * level) begins; the columns' ranks are searched inside the level's range, and one workgroup per (gene, level) runs
 * cna_gene_rank_corr's walk on its sub-segment with m_l cells, k_l stored entries and m_l - k_l implicit zeros.
 * work_bytes, the stream, the buffers and the states it may be called in: as cna_gene_rank_corr.  The same bits on every
 * run, under every work_bytes and for a CSR and a CSC upload of one matrix.
 * CNA_ESTATE: no expression matrix is resident.  CNA_EINVAL, with nothing written: a null pointer, q outside [1, 16],
 * n_bins outside [1, 255], a negative work_bytes, a code outside [-1, n_bins).  CNA_ENOMEM: the results do not fit on
 * the device. */
int  cna_gene_rank_corr_by(cna_ctx* ctx, const double* V, int q, const int32_t* codes, int n_bins, int64_t work_bytes,
                           uint64_t* s_lo_out, int64_t* s_hi_out, double* tie_gene_out, double* tie_key_out, int64_t* m_out,
                           uint8_t* nan_out);

/* ---- Spearman's rho under the permuted phenotypes (csrc/expr_rankperm.hip) -------------------- */
/* cna.tl.gene_rank_test: cna_gene_rank_corr against the null coefficients of the association's permuted phenotypes.  The
 * null coefficient of a conditioned, standardised null phenotype z_p is c_p = X z_p per cell (reference
 * _association.py:94-99, with X the residualised NAM; the observed one is _association.py:77).  Ranks are not linear in
 * z_p, so -- unlike cna_expr_cross, which serves the Pearson null from W = E^T X alone -- every c_p is formed, ranked and
 * correlated with every gene's ranks.  The three entries run on the expression stream with the work buffers of
 * cna_gene_ranksum_by (grow-only, freed by cna_expr_drop); X is read and left as it is (the expression stream waits for
 * what the main stream has queued that produces X, as in cna_expr_cross; cna_x_generation does not move).  Every argument
 * is judged before anything is written, and the caller's buffers are written only after everything has succeeded.
 *
 * The columns alone:
 *   Z[j * n_cols + s]   row j of q, 1 <= q <= 4096, one row per column to form; n_cols = the samples of X, <= 1024
 *   xrow[i]             the row of X of cell i of the expression matrix (CALLER's cell order, n_cells entries), -1 for a
 *                       cell that has none: cna_expr_cross's map, judged by its check with its verdicts and messages
 *   out[j * n_cells + i] = sum over s of X[xrow[i]][s] * Z[j][s] for xrow[i] >= 0, NaN where xrow[i] == -1
 * float64 throughout, the samples in ascending order, each product rounded on its own and then added to the running sum
 * (no fused multiply-add): the bits of `acc = zeros; for s: acc = acc + X[rows, s] * Z[j, s]` in numpy.
 * CNA_ESTATE: no expression matrix is resident, X not available, a communicator is active.  CNA_EINVAL: a null pointer,
 * another length than the matrix' cells, q or the samples of X out of range, a bad xrow.  CNA_ENOMEM: q x n_cells
 * float64 do not fit on the device. */
int  cna_x_columns(cna_ctx* ctx, const int64_t* xrow, int64_t n_cells, const double* Z, int q, double* out);
/* The integers of cna_gene_rank_corr for the q columns cna_x_columns forms, 1 <= q <= 4096, from ONE sort of the matrix.
 * The kept cells are those with xrow[i] >= 0 -- the set does not depend on the column -- so a formed value that is not
 * finite (an inf or a NaN in X or Z) is refused with CNA_EINVAL.  Outputs as cna_gene_rank_corr's: s_lo_out, s_hi_out
 * [q, n_genes], tie_gene_out [n_genes], tie_key_out [q], *m_out, nan_out [n_genes].
 * The columns go in groups of 16: formed into a 16 x n_cells buffer, ranked by cna_gene_rank_corr's passes, b = s + e - m
 * written to the group's own cell-major table [cell][16] of int32.  All tables stay resident: 64 x ceil(q / 16) x n_cells
 * bytes.  Then every tile of genes is sorted once (work_bytes as in cna_gene_rank_corr); behind it one workgroup per gene
 * walks its list forward and backward once and stores a = s + e - m per entry, and one workgroup per (gene, group)
 * streams {a, cell}, gathers the cell's 64-byte row and adds a x b per column in cna_gene_rank_corr's integer
 * accumulators.  For every group of 16 columns the results equal cna_gene_rank_corr's on those columns under the same kept
 * set, integer for integer, under every work_bytes and on every run.
 * CNA_ESTATE, CNA_EINVAL as cna_x_columns, and a negative work_bytes.  CNA_ENOMEM: the tables or the results do not fit. */
int  cna_gene_rank_corr_x(cna_ctx* ctx, const int64_t* xrow, int64_t n_cells, const double* Z, int q, int64_t work_bytes,
                          uint64_t* s_lo_out, int64_t* s_hi_out, double* tie_gene_out, double* tie_key_out, int64_t* m_out,
                          uint8_t* nan_out);
/* cna.tl.gene_rank_test_strata: cna_gene_rank_corr_x inside every level of a clustering, from the ONE sort of the matrix
 * and one table per group of 16 columns.  1 <= q <= 4096, 1 <= n_bins <= 255.
 *   codes[i]  the level of cell i in [0, n_bins), or -1: the cell is left out (judged as cna_gene_rank_corr_by judges them)
 * The kept cells of level l, C_l, are the cells with codes[i] == l and xrow[i] >= 0; genes and columns are ranked with
 * midranks inside C_l.
 *   s_lo_out, s_hi_out [(l * q + k) * n_genes + g]   S of level l, column k, gene g
 *   tie_gene_out[l * n_genes + g], tie_key_out[l * q + k]   the tie terms inside C_l
 *   m_out[l] = |C_l|
 *   nan_out[g]  a cell of ANY C_l holds NaN in gene g: cna_gene_rank_corr_by's guard on the whole gene (its other outputs
 *             are unspecified in every level)
 * Level l equals cna_gene_rank_corr_x called with xrow set to -1 outside level l, and every group of 16 columns equals
 * cna_gene_rank_corr_by on those columns of cna_x_columns(xrow, Z) under the same codes: integer for integer (s_lo, s_hi,
 * both tie terms and m), under every work_bytes and on every run.  A cell keeps its level where it has a row of X; every
 * group is ranked inside the levels (cna_gene_rank_corr_by's searches) with n_bins x 16 tie terms of its own; the genes'
 * sort ends on its pass on the level, the kernel that stores a runs once per (gene, level) on the level's sub-segment with
 * m_l cells, k_l stored entries and m_l - k_l implicit zeros, and the dot kernel once per (gene, group, level).  An empty
 * (gene, level) gives S = 0.  The results take 16 x n_bins x q x n_genes bytes on the device and on the host.
 * CNA_ESTATE, CNA_EINVAL as cna_gene_rank_corr_x; CNA_EINVAL, with nothing written, also for n_bins outside [1, 255] and a
 * code outside [-1, n_bins).  CNA_ENOMEM: the tables or the results do not fit. */
int  cna_gene_rank_corr_x_by(cna_ctx* ctx, const int64_t* xrow, int64_t n_cells, const double* Z, int q, const int32_t* codes,
                             int n_bins, int64_t work_bytes, uint64_t* s_lo_out, int64_t* s_hi_out, double* tie_gene_out,
                             double* tie_key_out, int64_t* m_out, uint8_t* nan_out);
/* The same core with the columns given by the host: V[k * n_cells + i], 1 <= q <= 4096.  The kept cells are those where
 * EVERY one of the q columns is finite: one set per call, as in cna_gene_rank_corr, found in a first pass over V before
 * any column is ranked.  Needs no X and no graph.  CNA_ESTATE: no expression matrix is resident.  CNA_EINVAL: a null
 * pointer, q outside [1, 4096], a negative work_bytes.  CNA_ENOMEM: the tables or the results do not fit. */
int  cna_gene_rank_corr_wide(cna_ctx* ctx, const double* V, int q, int64_t work_bytes, uint64_t* s_lo_out, int64_t* s_hi_out,
                             double* tie_gene_out, double* tie_key_out, int64_t* m_out, uint8_t* nan_out);

/* ---- the expression matrix against the working matrix (csrc/expr_cross.hip) ------------------- */
/* What cna.tl.gene_test needs from the cells: with c_p = X^T z_p / N the coefficient of a permuted, conditioned phenotype
 * z_p (_association.py:94-99; the observed one is _association.py:77 with z = the standardised y), the correlation of
 * gene g with c_p -- demo/demo.ipynb's "per-gene correlations to neighborhood coefficient" under the null -- needs
 *   sum_i x[i,g] c_p[i] = (W_g . z_p) / N,   sum_i c_p[i] = (rho . z_p) / N,   sum_i c_p[i]^2 = z_p^T (X^T X) z_p / N^2
 * so one contraction over the cells serves every permutation of every phenotype on the same covariates:
 *   W_out[g * n_cols + s] = sum over the cells i with xrow[i] >= 0 of x[i,g] * X[xrow[i]][s]      (n_genes x n_cols)
 *   rho_out[s] = sum over those cells of X[xrow[i]][s];  sx_out[g], sxx_out[g] = their sums of x[i,g] and x[i,g]^2
 *   *m_out = their number
 * X is the working matrix (CNA_MAT_X: rows x n_cols float64, n_cols <= 1024), read and left as it is; xrow[i] is the row
 * of X of cell i of the expression matrix (CALLER's cell order, n_cells entries), -1 for a cell that has none (the
 * selection dropped it).  xrow is checked on the device before any sum is formed: CNA_EINVAL, with nothing written, for a
 * value outside [-1, rows of X), a row of X named twice, or n_cells other than the resident matrix' cells.  CNA_ESTATE: no
 * expression matrix, no X, or a context with a communicator (the rows of other ranks are elsewhere).  The f32 state
 * switch (cna_set_state_f32) is supported: it concerns the walk's state only, X is float64 either way.
 * Sums are float64 in a fixed order (dense: the cells of a slab ascending, slabs in order; gene-major lists: a gene's
 * entries ascending, chunks in order; no floating-point atomics): two runs give the same bits, and so do a CSR and a CSC
 * upload of one matrix.  Runs on the expression stream with grow-only buffers of its own (freed by cna_expr_drop) and
 * changes no other state; it waits there, through an event, for what the main stream has queued that produces X, and
 * returns only after its own stream has drained, so a later producer of X finds the read finished.  May be called between cna_null_local_launch and cna_null_local_fetch (both read X). */
int  cna_expr_cross(cna_ctx* ctx, const int64_t* xrow, int64_t n_cells, double* W_out, double* rho_out, double* sx_out,
                    double* sxx_out, int64_t* m_out);
/* Counts the times the working matrix X and what is derived from it were voided (every producer of X, every transition
 * above it): a caller that keeps something derived from X (cna_expr_cross' result) may keep it while this stands still. */
int  cna_x_generation(cna_ctx* ctx, int64_t* gen);

/* ---- the same inside every level of a clustering (csrc/expr_cross_by.hip, csrc/gram_by.hip) ---- */
/* What cna.tl.gene_test_strata needs from the cells: the sums of cna_expr_cross over the cells of one level (cluster) at a
 * time, so that the correlation of gene g with the null coefficient c_p = X^T z_p / N (_association.py:94-99) inside level l
 * -- the question cna.pl.violinplot(d, 'leiden', key='coef') (plotting/_strat.py:21-29) raises -- is sample-space algebra:
 *   sum_{i in C_l} x[i,g] c_p[i] = (W_l[g] . z_p) / N,   sum c_p[i] = (rho_l . z_p) / N,   sum c_p[i]^2 = z_p^T Gamma_l z_p / N^2
 * codes[i] is the level of cell i (CALLER's cell order), -1 for a cell that is left out, 1 <= n_bins <= 1024; xrow[i] its
 * row of X as for cna_expr_cross.  A cell takes part in level codes[i] when codes[i] >= 0 and xrow[i] >= 0 (C_l).
 *
 * cna_expr_cross_by, for the levels [bin0, bin0 + nb) of n_bins, l = level - bin0:
 *   W_out[(l * n_genes + g) * n_cols + s] = sum over C_level of x[i,g] * X[xrow[i]][s]
 *   sx_out[l * n_genes + g], sxx_out[l * n_genes + g] = their sums of x[i,g] and x[i,g]^2;  m_out[l] = |C_level|
 * in one pass over the resident DENSE matrix; rho_l is cna_matrix_to_bins(CNA_MAT_X).  n_cells must equal the resident
 * matrix' cells.  A gene-major resident matrix is refused with CNA_ESTATE: a one-pass kernel for that form was measured
 * slower than one cna_expr_cross per level with xrow masked to the level (profiles/kbench_gene_test_strata.txt) and is not
 * in the library; Engine.expr_cross_by takes that route for it.
 *
 * cna_gram_by, for every level: gram_out[(l * n_cols + a) * n_cols + b] = sum over C_l of X[xrow[i]][a] * X[xrow[i]][b]
 * (symmetric: the upper triangle is computed on the f64 matrix cores and mirrored; all levels together do the flops of one
 * cna_gram, the NAM.dot(NAM.T) of _nam.py:105), m_out[l] = |C_l|.  It needs no resident expression matrix; 1 <= n_cells <
 * 2^31.  CNA_EINVAL when n_bins x n_cols^2 x 8 bytes exceed 1 GiB: take the levels in groups (cells of other levels -1).
 *
 * Both check xrow (as cna_expr_cross does) and the codes on the device before any sum is formed: CNA_EINVAL, with nothing
 * written, for an xrow outside [-1, rows of X), a row of X named twice, a code outside [-1, n_bins), or a count out of
 * range (n_bins, bin0, nb, n_cells, n_cols <= 1024) -- those before anything is queued.  CNA_ESTATE: no X, a context with a
 * communicator (the rows of other ranks are elsewhere), and for cna_expr_cross_by no resident dense expression matrix.
 * Sums are float64 in a fixed order (the cells of a level ascending, cut into chunks whose partials are added in chunk order;
 * no floating-point atomics): two runs give the same bits.  NaN / inf inside the expression matrix reach their own (level,
 * gene) only.  Both run on the expression stream with grow-only buffers of their own (freed by cna_expr_drop), read X and leave it
 * as it is, wait there through an event for what the main stream has queued that produces X, and return only after their
 * own stream has drained. */
int  cna_expr_cross_by(cna_ctx* ctx, const int64_t* xrow, const int32_t* codes, int64_t n_cells, int n_bins, int bin0, int nb,
                       double* W_out, double* sx_out, double* sxx_out, int64_t* m_out);
int  cna_gram_by(cna_ctx* ctx, const int64_t* xrow, const int32_t* codes, int64_t n_cells, int n_bins, double* gram_out,
                 int64_t* m_out);

/* ---- the NAM or the working matrix by bin (csrc/nam_bins.hip) ---------------------------------- */
/* "Working directly with the NAM" (demo/demo.ipynb, section 3.2) and the plot every analysis ends on -- the phenotype against
 * the abundance of the associated population in each sample -- need sums over the cell axis of the NAM (_nam.py:73), per
 * cluster and per weight column; the reference takes the NAM to the host for them and aggregates as utils/multisample.py:4-11
 * aggregates per-cell columns.  Here the matrix stays where it is: one read of it, weights x bins x samples out.
 *   which     CNA_MAT_NAM or CNA_MAT_X
 *   codes[r]  the bin of LOCAL ROW r of that matrix (the device's row order, as for cna_fetch_rows and cna_load_cell_stat),
 *             -1 for a row that is left out; n_rows must equal the rows cna_matrix_shape reports; 1 <= n_bins <= 1024
 *   W         q x n_rows row-major weights, 0 <= q <= 16, or NULL with q = 0: every weight 1; max(q, 1) x n_bins <= 4096
 * Row r CONTRIBUTES to weight column j when codes[r] >= 0 and W[j][r] is finite and not zero (q = 0: when codes[r] >= 0).  A
 * row that does not contribute is not multiplied at all: a zero weight against a NaN entry of the matrix adds nothing.
 *   sums_out[(j * n_bins + L) * n_cols + s] = sum over the contributing rows r of bin L of W[j][r] * M[r][s], n_cols as
 *   cna_matrix_shape reports it (the padding up to the leading dimension never appears)
 *   n_out[j * n_bins + L] = the number of those rows
 * (one weight column and n_bins rows of each with q = 0).  A bin without contributing rows gives 0; NaN / inf inside the
 * matrix reach their own (j, bin, column) only.  Sums are float64 in a fixed order (the rows of a bin ascending, cut into
 * chunks whose partials are added in chunk order; no floating-point atomics): two runs give the same bits.  The product is
 * fused: sum = fma(w, x, sum), one rounding per row.
 * CNA_MAT_NAM collects a pending cna_nam_auto_launch verdict and produces a NAM that cna_nam_select_hint's by-product left
 * lazy, as cna_fetch_rows does.  The matrix is read and left as it is and nothing derived from it is kept.  Runs on the
 * expression stream with grow-only buffers of its own (freed by cna_expr_drop), needs no resident expression matrix, waits
 * there, through an event, for what the main stream has queued that produces the matrix, and returns only after its own
 * stream has drained, so a later producer finds the read finished.
 * CNA_ESTATE: the matrix is not available, or the context has a communicator (the rows of other ranks are elsewhere).
 * CNA_EINVAL, with nothing written: which, q, n_bins or n_rows out of range, or a code outside [-1, n_bins) -- found on the
 * device before any sum is formed. */
int  cna_matrix_to_bins(cna_ctx* ctx, int which, const int32_t* codes, const double* W, int q, int64_t n_rows, int n_bins,
                        double* sums_out, int64_t* n_out);

/* ---- gene set enrichment of the gene correlations (csrc/enrich.hip) ---------------------------- */
/* demo/demo.ipynb, section 1.5, ends the per-gene correlations to the neighbourhood coefficient with "they could be further
 * analyzed using techniques like gene set enrichment analysis".  This is that analysis' cell-free core, for the variant
 * that permutes the phenotype: the extremes of the running sum of every gene set under every column of [r | null_r], the
 * null columns being the correlations under the association's own conditional permutations (_association.py:94-99, as
 * cna.tl.gene_test forms them).
 *   R          n_cols x n_genes row-major, one row per phenotype column (the observed r first); 1 <= n_cols <= 4096,
 *              1 <= n_genes < 2^31
 *   set_ptr    n_sets + 1 offsets into set_genes, starting at 0, not falling; 1 <= n_sets <= 2^20, at most 4096 members per
 *              set, fewer than 2^31 in all
 *   set_genes  the members' gene indices, in [0, n_genes) and strictly ascending inside a set
 *   weight     0, 1 or 2: the exponent p of w = |r|^p, evaluated as 1, fabs(r), r * r (a product rounded on its own).  Other
 *              exponents are refused: pow rounds differently in libm and on the device
 * For column c a gene is VALID when R[c][g] is finite; valid_out[c] = Gv, their number.  The position of a valid gene is
 *   pos(g) = #{valid h : r_h > r_g} + #{valid h < g : r_h == r_g}
 * -- its place in np.argsort(-r, kind='stable') over the valid genes; +0.0 and -0.0 tie.  For set s take its valid members in
 * order of position, j = 1 .. k, with w_j their weight, S_j = w_1 + ... + w_j, N_R = S_k and m_j = pos_j - (j - 1) the misses
 * before hit j:
 *   up_out[c * n_sets + s]   = max_j  S_j / N_R - (double)m_j / (double)(Gv - k)
 *   down_out[c * n_sets + s] = min_j  S_(j-1) / N_R - (double)m_j / (double)(Gv - k)
 *   size_out[c * n_sets + s] = k
 * two divisions and one subtraction each, in exactly this form.  Both are NaN when k == 0, k == Gv or N_R == 0; otherwise
 * up >= 0 >= down.  The enrichment score, ES = up if up >= -down else down, is left to the caller: a near-tie of the two
 * extremes cannot turn one rounding into a sign flip here, and both tails are available.
 * The positions are integer counts over all pairs of genes of a column (exact, ties by construction); S_j is added in a
 * fixed order and the extremes are folded by fmax / fmin; no floating-point atomics: two runs give the same bits.
 * Like cna_coef_strata it needs no graph and no resident expression matrix and changes no other state; it runs on the
 * expression stream with grow-only buffers of its own (freed by cna_expr_drop; 12 bytes per entry of R) and returns after that
 * stream has drained.
 * CNA_EINVAL, with nothing written: a limit above violated, a weight other than 0, 1, 2, or a member out of range or out of
 * order -- found on the device before any sum is formed. */
int  cna_enrichment_extremes(cna_ctx* ctx, const double* R, int64_t n_cols, int64_t n_genes, const int64_t* set_ptr,
                             const int32_t* set_genes, int n_sets, int weight, double* up_out, double* down_out,
                             int32_t* size_out, int32_t* valid_out);

/* ---- the coefficient on the embedding, as images (csrc/raster.hip) ---------------------------- */
/* The picture the reference's workflow draws right after cna.tl.association, as numbers:
 *     cna.pl.umap_ncorr(d, key='case_coef')                  (demo/demo.ipynb 1.2 and 1.3; plotting/_umap.py:6-36)
 * draws every cell in grey and on top the cells with coef_fdr <= 0.1 coloured by coefficient, scanpy sorting the points so
 * that the highest lies on top; demo 3.2.1 draws sc.pl.umap(d, color='NAMPC1', cmap='seismic') the same way without an
 * fdr.  Here the cells are reduced to the pixels of a width x height grid over the embedding, ready for Axes.imshow.
 *   xy        n_cells x 2 float64 (x, y), CALLER's cell order, n_cells in [1, 2^31)
 *   V         q x n_cells row-major, 1 <= q <= 16: the value of every cell under every key
 *   FDR       q x n_cells row-major; row k is read only where has_fdr[k] != 0 (FDR may be NULL when no key has one)
 *   extent    {x0, x1, y0, y1}.  auto_extent = 0: read; finite with x1 > x0 and y1 > y0.  auto_extent != 0: written, the
 *             minimum and maximum of x and of y over the cells where both are finite (found on the device, order-free and
 *             exact); an axis whose minimum equals its maximum v becomes [v - 0.5, v + 0.5], as np.histogram widens it.
 *             With no such cell at all extent becomes four NaN, the call returns 0 and writes nothing else.
 *   width, height in [1, 4096] with q * width * height <= 2^22; radius in [0, 16]
 * The pixel rule.  sx = (double)width / (x1 - x0), sy = (double)height / (y1 - y0), each evaluated once on the host.  A
 * cell is INSIDE when x and y are finite, x0 <= x <= x1 and y0 <= y <= y1; then t = (x - x0) * sx, one subtraction and one
 * multiplication each rounded on its own, ix = (int64)floor(t), and x == x1 or a rounded ix >= width give width - 1; iy
 * likewise from y0, sy and height.  Images are [iy * width + ix], row 0 at y0 (imshow's origin='lower').
 * A cell PASSES for key k when V[k] is finite and, where has_fdr[k], FDR[k] <= fdr_thresh (a NaN fdr fails).
 *   n_out[height * width]            inside cells, whatever their values (the grey layer)
 *   *n_outside_out                   cells with finite coordinates that are not inside
 *   n_pass_out[q * height * width]   inside cells that pass
 *   sum_out                          their sum, 0 where none passes
 *   top_out, bottom_out              their largest (what sort_order=True leaves visible) and smallest value, NaN where
 *                                    none passes; +0.0 and -0.0 compare equal, which sign comes back is not specified
 *   absmax_out[q]                    max |V[k]| over the inside cells that pass (vmin / vmax of _umap.py:27-28), NaN if none
 *   covered_out[height * width]      (may be NULL) 1 where a pixel within the disc (ix - ix')^2 + (iy - iy')^2 <= radius^2
 *                                    has n > 0, else 0
 * radius > 0 (the marker size s of the scatter) replaces top_out / bottom_out by their dilations with the same disc: the
 * maximum of top, the minimum of bottom over the disc's pixels inside the image, pixels where nothing passes ignored.  The
 * counts and the sums stay per pixel.
 * Counts, top, bottom, absmax and the extent are exact.  sum is float64 in a fixed order that does not depend on
 * scheduling (the passing cells of a pixel ascending in the cell index, cut into chunks whose partials are added in chunk
 * order; no floating-point atomics): two runs give the same bits, and a pixel that holds most of the cells is spread over
 * as many wavefronts as it has chunks.
 * Like cna_coef_strata it needs no graph and no resident expression matrix and changes no other state; it may be called
 * between cna_null_local_launch and cna_null_local_fetch, runs on the expression stream with grow-only buffers of its own
 * (freed by cna_expr_drop) and returns after that stream has drained.
 * CNA_EINVAL, with nothing written: a side outside [1, 4096], q outside [1, 16], q * width * height > 2^22, radius outside
 * [0, 16], n_cells outside [1, 2^31), an explicit extent that is not finite or not increasing. */
int  cna_coef_raster(cna_ctx* ctx, const double* xy, const double* V, const double* FDR, const int32_t* has_fdr, int q,
                     int64_t n_cells, double fdr_thresh, double* extent, int auto_extent, int width, int height, int radius,
                     int64_t* n_out, int64_t* n_outside_out, int64_t* n_pass_out, double* sum_out, double* top_out,
                     double* bottom_out, uint8_t* covered_out, double* absmax_out);

/* ---- connected populations of the resident graph (csrc/components.hip) ------------------------ */
/* What the reference's demo says in words after cna.tl.association (demo/demo.ipynb 1.3: "a sub-population of the left-hand
 * cluster", "these cells comprise only ~6 % of the cells that pass the threshold"), as data: the connected groups of cells
 * of one class in the kNN graph that cna_graph_upload made resident (_nam.py:12-19 is where the reference reads it).
 *   codes      int32 per cell, CALLER's cell order: a class in [0, n_classes) or -1 for none; n_cells = the graph's cells
 * Two classed cells belong to one component when a chain of stored entries joins them, read in either direction, every
 * cell on the chain being of their class (weak connectivity; self loops and duplicates change nothing).  An entry is an
 * edge whatever its value, a stored zero included: the values of the graph are not read.
 * cna_graph_components_find runs a lock-free union-find on the device (hooking by compare-and-swap on roots, path
 * shortening by atomic minimum, no thread ever waits for another), flattens it and counts the same-class entries whose
 * ends still have different roots; while that count is not zero it repeats from the current state, 32 rounds at most
 * (CNA_ESTATE beyond).  Then the size and the smallest caller index of every component by integer atomics.
 *   *n_kept_out   the components with at least min_cells cells
 *   totals_out    [n_classes]: the components of every class, before that filter
 *   *sweeps_out   rounds taken, >= 1
 * cna_graph_components_list copies the kept components out: class, size, smallest caller cell index, n_kept each, in the
 * order in which they arrived on the device -- NOT a fixed one: sort them.
 * cna_graph_components_label writes comp_out[cell] (caller's order, int32): rank[j] for a cell of the component at place j
 * of that list (rank = NULL: j itself; else a permutation's values in [0, n_kept)), -1 for a cell without a class or of a
 * component below min_cells.
 * One rank holding the whole graph (CNA_ESTATE otherwise).  The three read the graph and the device's cell order and
 * write only buffers of their own (freed by cna_expr_drop, after which _list and _label want a new _find; likewise after
 * a new graph or cell order): the walk, the NAM, X and everything derived from them stay valid.  They run on the expression
 * stream behind whatever the main stream has queued and return once their stream has drained.  No floating point. */
int  cna_graph_components_find(cna_ctx* ctx, const int32_t* codes, int64_t n_cells, int n_classes, int64_t min_cells,
                               int64_t* n_kept_out, int64_t* totals_out, int* sweeps_out);
int  cna_graph_components_list(cna_ctx* ctx, int64_t n_kept, int32_t* class_out, int32_t* size_out, int32_t* first_out);
int  cna_graph_components_label(cna_ctx* ctx, const int32_t* rank, int64_t n_kept, int32_t* comp_out, int64_t n_cells);

/* ---- neighbourhood-mean expression (csrc/expr_nbhd.hip) ---------------------------------------- */
/* The gene side in the unit of the association's result.  cna.tl.association's coefficient is a number per
 * NEIGHBOURHOOD: neighbourhood i is the soft set of cells that the nsteps-step random walk anchored at cell i reaches
 * (_nam.py:21-41), and the NAM is the abundance of every sample in those sets (_nam.py:44-76).  With one step of that walk
 *     c = A.sum(axis=0) + w                 (_nam.py:28)
 *     P s = A.(s/c) + w*s/c                  (_nam.py:33)
 * and e_g the column of gene g of the resident expression matrix widened to float64,
 *     m_g = (P^nsteps e_g) / (P^nsteps 1)    element-wise
 * is the mean of the gene over neighbourhood i with the weights the NAM uses: the numerator is what the NAM would hold if
 * the gene were a sample, the denominator the neighbourhood's total membership mass.  A cell whose denominator is not a
 * positive finite number is left out of every sum and its m is NaN.  w is the self weight of the last cna_colsums.
 * The numerators and the denominator are, bit for bit, what cna_dense_load / nsteps x cna_dense_step / cna_dense_fetch
 * return for the same columns on the same context (float32 and float64 graphs, any device cell order): the quotient s/c
 * first, a row's stored entries in stored order, a multiply and then an add, no contraction.
 *
 * Both read the graph, the device's cell order and the column sums where they are and write only buffers of their own
 * (freed by cna_expr_drop): the walk's state, the NAM, X and everything derived from them stay valid -- the NAM an
 * association cached survives a call, and a call between the launch and the fetch of a local-null pass is fine.  They run on
 * the expression stream behind whatever the main stream has queued and return once it has drained.
 * CNA_ESTATE: no graph, no cna_colsums, no resident expression matrix, or a context with a communicator / a row block.
 * CNA_EINVAL: the graph and the matrix differ in their cells; nsteps outside [1, 15]; q outside [1, 16]; m outside
 * [1, 64] or a gene outside [0, n_genes).  CNA_ENOMEM: the tile buffers (2 x n_cells x 64 float64 and the per-cell
 * columns) do not fit; nothing of the call is resident afterwards.
 *
 * cna_nbhd_expr: genes int32[m]; num_out n_cells x m row-major and den_out n_cells, float64, CALLER's cell order. */
int  cna_nbhd_expr(cna_ctx* ctx, const int32_t* genes, int m, int nsteps, double* num_out, double* den_out);
/* cna_gene_nbhd_corr: V as for cna_gene_corr (q x n_cells row-major, caller's cell order, NaN = cell left out).  Per gene
 * and key over the cells where the key is finite and the denominator good (each key its own set; n_cells_out[j] of them):
 *   r_out[j * n_genes + g]     Pearson correlation of m_g with column j, clipped to [-1, 1]
 *   mean_out, sd_out           mean and population sd of m_g over those cells (same layout)
 * in two passes over the tile while it is resident -- sum m; then sum (m - mean)^2 and sum (m - mean)(v - mean v) -- with
 * partial sums per slab of rows added in slab order (no floating-point atomics: the same bits on every run).  r is NaN
 * where numpy's 0 / 0 gives NaN (a constant key, fewer than two cells) and for a gene that is constant over ALL cells of the
 * raw matrix, decided exactly: minimum == maximum with the implicit zeros counted.  times_ms_out: NULL, or 3 doubles
 * that receive the milliseconds spent filling tiles, walking and on the moments (the stream is then drained between
 * the phases: for measurements). */
int  cna_gene_nbhd_corr(cna_ctx* ctx, const double* V, int q, int nsteps, double* r_out, double* mean_out, double* sd_out,
                        int64_t* n_cells_out, double* times_ms_out);

/* ---- measurement ------------------------------------------------------------------------ */
/* HIP-event timing of every kernel launch on the context's stream (bench.py roofline).  on = 1: every kernel group;
 * on = 2: the walk kernels (CNA_K_NAM_FIRST / _STEP / _STEP_SPARSE) and the communication spans only -- two event records
 * per span cost the host ~0.1 ms of a 1.2 ms analysis when all ~20 groups are timed; 0: off. */
int  cna_prof_enable(cna_ctx* ctx, int on);
int  cna_prof_reset(cna_ctx* ctx);
int  cna_prof_get(cna_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches);
const char* cna_kernel_name(int kernel_id);

/* svd_nam's `np.linalg.svd(NAM.dot(NAM.T))` (_nam.py:105) as the global test consumes it (_association.py:35-48: the
 * first k <= max(ks) vectors, through squared projections only): the k leading eigenpairs of the symmetric n x n matrix
 * G (row-major) on the host -- Householder tridiagonalisation, bisection, inverse iteration (csrc/host_eig.c) -- with
 * the evidence the caller needs to accept them or fall back to LAPACK: U_out n x k row-major (column t belongs to the
 * t-th largest eigenvalue, sign arbitrary), lam_out the k + 1 largest eigenvalues, *resid_out / *ortho_out = largest
 * residual and largest orthogonality defect of the eigenvectors of the tridiagonal stage (the one that can fail; the
 * reflectors around it are orthogonal to rounding).  Returns 0; 1 = breakdown, 2 = bad arguments (k + 1 <= min(n, 260)),
 * -1 = no memory.  Needs no context and no GPU. */
int  cna_host_top_eig(const double* G, int n, int k, double* U_out, double* lam_out, double* resid_out, double* ortho_out);
/* The same two figures measured on G itself: max_t ||G u_t - lam_t u_t||_inf, max |U^T U - I| (tests). */
int  cna_host_eig_check(const double* G, int n, int k, const double* U, const double* lam, double* resid_out, double* ortho_out);

#ifdef __cplusplus
}
#endif
#endif /* CNA_HIP_H */

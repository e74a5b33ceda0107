// Per-gene Pearson correlation to per-cell columns (the neighbourhood coefficient of cna.tl.association, NAM PC
// loadings, ...) over an expression matrix that stays resident on the device.  Replaces the host line of the
// reference's workflow (demo/demo.ipynb, "per-gene correlations to neighborhood coefficient"):
//     d.var['corr_case'] = np.corrcoef(d.obs.male_coef.values.reshape(1,-1), d.X, rowvar=False)[0,1:]
//
// Nothing here writes the state of c_api.hip (graph, walk, NAM, X, cell order), and only cna_expr_cross reads any of it
// (the working matrix X, read-only): the matrix and the key columns are in the CALLER's cell order, the buffers and the
// stream are this file's own (cna_ctx::expr).
//
//   k_key_stats     per key column: finite count, mean, sum (v - mean), sum (v - mean)^2, min, max (fixed-order sums)
//   k_key_table     cells x Q table of centred key values (0 where the cell is left out) + one mask word per cell
//   k_gc_dense      X is cells x genes: lane = gene, a wave walks down a slab of cells (coalesced rows, the key values
//                   of a cell are wave-uniform); partial sums per slab with plain stores
//   k_gc_sparse     gene-major lists {cell, value}: one wave per chunk of a gene's list, gathers the cell's table row;
//                   partial sums per chunk with plain stores
//   k_gc_finish_*   adds the partials of a gene in slab / chunk order and turns them into r
//   k_tr_*          counting transpose of a CSR upload into the gene-major form, stable in the cell index
//
// Per-bin sums of the same resident matrix (cna.ut.expr_to_sample: the samples x genes "pseudobulk" that stands beside
// the reference's utils/multisample.py:4-11 obs_to_sample), cna_expr_to_bins:
//   k_pb_count      checks every code against [-1, n_bins) and counts the cells of every bin per block of cells
//                   (integer atomics in LDS); k_tr_scan turns the counts into offsets
//   k_pb_fill       the cells sorted by bin, ascending inside a bin whatever the scheduling: a wave takes 64 cells at a
//                   time in order and ranks equal codes by lane (dense form only: the lists carry their cell already)
//   k_pb_dense      lane = gene, a workgroup walks a chunk (PB_DENSE_CHUNK cells) of one bin's cell list, every row read
//                   a coalesced run of genes; one partial per (chunk, gene) with plain stores
//   k_pb_sparse     one wave per chunk of a gene's list, the bins' accumulators in LDS (4096 doubles at most); lanes of
//                   one batch that meet in a bin are served lowest lane first, in rounds (an integer LDS atomic names
//                   the lane whose turn it is); one partial per (chunk, bin) with plain stores
//   k_pb_finish_*   adds the partials of a (bin, gene) in chunk order
// Partial storage: dense (cells / PB_DENSE_CHUNK + min(cells, n_bins)) x genes doubles -- never more than the result plus
// 1 / 1024 of the matrix' own size (f32); gene-major lists: chunks x n_bins doubles, held to PB_PART_BYTES (256 MB) by
// going over the genes in tiles (a single gene whose chunks alone exceed it gets a tile of its own: at most 2^31 / 65536
// chunks x 4096 bins x 8 bytes = 1 GB).
//
//
// The expression matrix against the working matrix X (cna.tl.gene_test), cna_expr_cross: W = E_K^T X, genes x samples,
// the one cell-sized contraction behind the null correlations of every gene with the permuted phenotypes' coefficients
// c_p = X^T z_p / N (the reference's null of _association.py:94-99; the observed coefficient is its line 77, and the
// per-gene correlation demo/demo.ipynb's "per-gene correlations to neighborhood coefficient"):
//   k_xc_check      every xrow against [-1, rows of X), every X row named at most once (integer atomics on a table of
//                   rows), the cells that take part counted -- judged on the host before any sum is formed
//   k_xc_dense      lane = gene, a wave walks a slab of cells for a tile of 32 samples: the row X[xrow[cell]] is the same
//                   in every lane (scalar loads), the product an FMA with one uniform operand; one partial per (slab,
//                   gene, sample) with plain stores.  The first tile also takes sum x and sum x^2
//   k_xc_sparse     one wave per chunk of a gene's list, lane = sample (ceil(n_cols / 64) accumulators per lane): 64
//                   entries are read at a time and handed round, the row X[xrow[cell]] is gathered coalesced
//   k_xc_rho        column sums of the rows of X that take part, per slab of cells
//   k_xc_finish_*   add the partials in slab / chunk order
//
// Result sums take a fixed order (no floating-point atomics): two runs on one input give the same bits.  Integer
// atomics only count and hand out cursors.
#include "common.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

namespace {

constexpr int GC_MAXQ = 16;
constexpr int KS_LD = 8;   // doubles per key in the key statistics block: n, mean, sum vc^2, sum vc, min, max

using Buf = DevBuf;

struct ExprState {
  hipStream_t st = nullptr;
  int format = 0;   // 0: none, 1: dense cells x genes, 2: gene-major lists
  int is_f64 = 0;
  int64_t n = 0, G = 0, nnz = 0;
  int64_t n_uploads = 0;
  Buf X;                           // dense
  Buf gptr, gcell, gval;           // gene-major: G + 1 offsets, cell of every entry (ascending inside a gene), values
  Buf chunk_lo, chunk_gene, gchunk;   // first entry / gene of every chunk; first chunk of every gene (G + 1)
  int64_t nchunks = 0, chunk_len = 0;
  // per call (grow-only until the matrix is dropped)
  Buf vraw, vtab, vmask, kstat, part, rout, flag;
  // cna_expr_to_bins: codes, per-block counts -> offsets, totals, the cell list, the chunks of the bins
  Buf bcode, bcnt, btot, blist, bptr, brng, bfirst;
  // cna_expr_cross: xrow, the table of named X rows, partial sums (W | sum x, sum x^2 | column sums), the results
  Buf xrow, xseen, xpart, xpart2, xrpart, xout;
  hipEvent_t x_ready = nullptr;    // main stream -> expression stream: what was queued there that produces X is done
  std::vector<int64_t> gchunk_h;   // host copy of gchunk (tiles over genes)
};

inline ExprState* state_of(cna_ctx* c) { return static_cast<ExprState*>(c->expr); }

int buf_free(cna_ctx* c, Buf& b) { return devbuf_free(c, b); }
int buf_need(cna_ctx* c, ExprState* s, Buf& b, int64_t bytes) { return devbuf_need(c, s->st, b, bytes); }

void release_matrix(cna_ctx* c, ExprState* s) {
  (void)hipStreamSynchronize(s->st);
  for (Buf* b : {&s->X, &s->gptr, &s->gcell, &s->gval, &s->chunk_lo, &s->chunk_gene, &s->gchunk, &s->vraw, &s->vtab,
                 &s->vmask, &s->kstat, &s->part, &s->rout, &s->flag, &s->bcode, &s->bcnt, &s->btot, &s->blist, &s->bptr, &s->brng,
                 &s->bfirst, &s->xrow, &s->xseen, &s->xpart, &s->xpart2, &s->xrpart, &s->xout})
    buf_free(c, *b);
  s->gchunk_h.clear();
  s->format = 0;
  s->n = s->G = s->nnz = 0;
  s->nchunks = s->chunk_len = 0;
}

int get_state(cna_ctx* c, ExprState** out) {
  if (!c->expr) {
    ExprState* s = new ExprState();
    hipError_t e = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->x_ready, hipEventDisableTiming);
    if (e != hipSuccess) {
      if (s->st) (void)hipStreamDestroy(s->st);
      if (s->x_ready) (void)hipEventDestroy(s->x_ready);
      delete s;
      cna_set_error(std::string("hipStreamCreate: ") + hipGetErrorString(e));
      return (int)e;
    }
    c->expr = s;
  }
  *out = state_of(c);
  return 0;
}

// ------------------------------------------------------------------ key columns
__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// one block of 1024 threads per key: thread t adds the cells t, t + 1024, ...; the 1024 partial sums are folded by a
// fixed tree -- the same bits on every run
__global__ __launch_bounds__(1024) void k_key_stats(const double* __restrict__ V, int64_t n, double* __restrict__ ks) {
  __shared__ double sh[4][1024];
  const int j = blockIdx.x, t = threadIdx.x;
  const double* v = V + (int64_t)j * n;
  double cnt = 0, sum = 0, mn = INFINITY, mx = -INFINITY;
  for (int64_t i = t; i < n; i += 1024) {
    const double x = v[i];
    if (finite_d(x)) {
      cnt += 1.0;
      sum += x;
      mn = fmin(mn, x);
      mx = fmax(mx, x);
    }
  }
  sh[0][t] = cnt; sh[1][t] = sum; sh[2][t] = mn; sh[3][t] = mx;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if (t < w) {
      sh[0][t] += sh[0][t + w];
      sh[1][t] += sh[1][t + w];
      sh[2][t] = fmin(sh[2][t], sh[2][t + w]);
      sh[3][t] = fmax(sh[3][t], sh[3][t + w]);
    }
    __syncthreads();
  }
  const double N = sh[0][0], mean = N > 0 ? sh[1][0] / N : 0.0, vmin = sh[2][0], vmax = sh[3][0];
  __syncthreads();
  double s1 = 0, s2 = 0;
  for (int64_t i = t; i < n; i += 1024) {
    const double x = v[i];
    if (finite_d(x)) {
      const double d = x - mean;
      s1 += d;
      s2 += d * d;
    }
  }
  sh[0][t] = s1; sh[1][t] = s2;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if (t < w) {
      sh[0][t] += sh[0][t + w];
      sh[1][t] += sh[1][t + w];
    }
    __syncthreads();
  }
  if (t == 0) {
    double* o = ks + j * KS_LD;
    o[0] = N; o[1] = mean; o[2] = sh[1][0]; o[3] = sh[0][0]; o[4] = vmin; o[5] = vmax; o[6] = 0; o[7] = 0;
  }
}

// cell-major table: one gather brings all Q centred values of a cell.  flag |= 1 when the keys' masks differ in a cell.
__global__ __launch_bounds__(256) void k_key_table(const double* __restrict__ V, int64_t n, int q, int Q,
                                                   const double* __restrict__ ks, double* __restrict__ tab,
                                                   uint32_t* __restrict__ mask, int* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t m = 0;
  for (int j = 0; j < Q; ++j) {
    double vc = 0.0;
    if (j < q) {
      const double x = V[(int64_t)j * n + i];
      if (finite_d(x)) {
        vc = x - ks[j * KS_LD + 1];
        m |= 1u << j;
      }
    }
    tab[i * Q + j] = vc;
  }
  mask[i] = m;
  if (m != 0 && m != (q >= 32 ? ~0u : (1u << q) - 1u)) atomicOr(flag, 1);
}

// ------------------------------------------------------------------ dense
// Field order of a partial record (F = 4 S + Q doubles, S = 1 when the keys share one mask, else Q):
//   [s]: sum x   [S + s]: sum x^2   [2S + s]: min x   [3S + s]: max x   [4S + j]: sum x (v_j - mean_j)
template <typename T, int Q, bool SHARED>
__global__ __launch_bounds__(64) void k_gc_dense(const T* __restrict__ X, int64_t n, int64_t G, int64_t slab_rows,
                                                 const double* __restrict__ tab, const uint32_t* __restrict__ mask,
                                                 double* __restrict__ part) {
  constexpr int S = SHARED ? 1 : Q;
  constexpr int F = 4 * S + Q;
  constexpr int U = 8;
  const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool act = g < G;
  const int64_t gl = act ? g : G - 1;          // idle lanes of the last gene block reload its last gene; nothing is stored
  const int64_t r0 = (int64_t)blockIdx.y * slab_rows;
  const int64_t r1 = r0 + slab_rows < n ? r0 + slab_rows : n;
  double sx[S], sxx[S], sxv[Q];
  T mn[S], mx[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    sx[s] = 0; sxx[s] = 0;
    mn[s] = (T)INFINITY; mx[s] = (T)-INFINITY;
  }
#pragma unroll
  for (int j = 0; j < Q; ++j) sxv[j] = 0;
  for (int64_t r = r0; r < r1; r += U) {
    T xs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t rr = r + u < r1 ? r + u : r1 - 1;
      xs[u] = X[rr * G + gl];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (r + u >= r1) break;
      const uint32_t m = mask[r + u];          // wave-uniform: a scalar load and a scalar branch
      if (m == 0) continue;
      const double* v = tab + (r + u) * Q;
      const double x = (double)xs[u];
      if (SHARED) {
        sx[0] += x;
        sxx[0] = fma(x, x, sxx[0]);
        mn[0] = xs[u] < mn[0] ? xs[u] : mn[0];
        mx[0] = xs[u] > mx[0] ? xs[u] : mx[0];
#pragma unroll
        for (int j = 0; j < Q; ++j) sxv[j] = fma(x, v[j], sxv[j]);
      } else {
#pragma unroll
        for (int j = 0; j < Q; ++j) {
          if (m >> j & 1) {
            sx[j] += x;
            sxx[j] = fma(x, x, sxx[j]);
            mn[j] = xs[u] < mn[j] ? xs[u] : mn[j];
            mx[j] = xs[u] > mx[j] ? xs[u] : mx[j];
            sxv[j] = fma(x, v[j], sxv[j]);
          }
        }
      }
    }
  }
  if (!act) return;
  double* o = part + (int64_t)blockIdx.y * F * G + g;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    o[(int64_t)(s)*G] = sx[s];
    o[(int64_t)(S + s) * G] = sxx[s];
    o[(int64_t)(2 * S + s) * G] = (double)mn[s];
    o[(int64_t)(3 * S + s) * G] = (double)mx[s];
  }
#pragma unroll
  for (int j = 0; j < Q; ++j) o[(int64_t)(4 * S + j) * G] = sxv[j];
}

// r of one (gene, key) from its sums.  cnt: entries that were added (dense: every kept cell; gene-major lists: the
// stored ones -- the others are zeros).  Constant genes and keys are decided exactly: minimum == maximum.
__device__ __forceinline__ double gc_r(double sx, double sxx, double mn, double mx, double cnt, double sxv,
                                       const double* __restrict__ ks) {
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double N = ks[0];
  if (N < 2.0) return nan;
  if (cnt < N) {
    mn = fmin(mn, 0.0);
    mx = fmax(mx, 0.0);
  }
  if (!(ks[4] < ks[5]) || mn == mx) return nan;
  const double mean = sx / N;
  const double varx = sxx - sx * mean;
  const double cov = sxv - mean * ks[3];
  double r = cov / sqrt(varx) / sqrt(ks[2]);
  if (r > 1.0) r = 1.0;
  if (r < -1.0) r = -1.0;
  return r;
}

__global__ __launch_bounds__(256) void k_gc_finish_dense(const double* __restrict__ part, int64_t G, int nslab, int q, int Q,
                                                         int S, const double* __restrict__ ks, double* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int F = 4 * S + Q;
  double sx = 0, sxx = 0, mn = INFINITY, mx = -INFINITY;
  for (int j = 0; j < q; ++j) {
    const int s = S == 1 ? 0 : j;
    if (j == 0 || S != 1) {
      sx = 0; sxx = 0; mn = INFINITY; mx = -INFINITY;
      for (int p = 0; p < nslab; ++p) {
        const double* o = part + (int64_t)p * F * G + g;
        sx += o[(int64_t)s * G];
        sxx += o[(int64_t)(S + s) * G];
        mn = fmin(mn, o[(int64_t)(2 * S + s) * G]);
        mx = fmax(mx, o[(int64_t)(3 * S + s) * G]);
      }
    }
    double sxv = 0;
    for (int p = 0; p < nslab; ++p) sxv += part[((int64_t)p * F + 4 * S + j) * G + g];
    out[(int64_t)j * G + g] = gc_r(sx, sxx, mn, mx, ks[j * KS_LD], sxv, ks + j * KS_LD);
  }
}

// ------------------------------------------------------------------ gene-major lists
__device__ __forceinline__ double wave_min_any(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max_any(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// Field order of a chunk's record (F = 5 S + Q doubles): as in the dense kernel, then [4S + s]: entries added,
// [5S + j]: sum x (v_j - mean_j)
template <typename T, int Q, bool SHARED>
__global__ __launch_bounds__(256) void k_gc_sparse(const int64_t* __restrict__ chunk_lo, const int32_t* __restrict__ chunk_gene,
                                                   const int64_t* __restrict__ gptr, int64_t nchunks, int64_t chunk_len,
                                                   const int32_t* __restrict__ gcell, const T* __restrict__ gval,
                                                   const double* __restrict__ tab, const uint32_t* __restrict__ mask,
                                                   double* __restrict__ part) {
  constexpr int S = SHARED ? 1 : Q;
  constexpr int F = 5 * S + Q;
  const int64_t ch = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (ch >= nchunks) return;
  const int64_t lo = chunk_lo[ch];
  const int64_t end = gptr[chunk_gene[ch] + 1];
  const int64_t hi = lo + chunk_len < end ? lo + chunk_len : end;
  double sx[S], sxx[S], mn[S], mx[S], cnt[S], sxv[Q];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    sx[s] = 0; sxx[s] = 0; cnt[s] = 0;
    mn[s] = INFINITY; mx[s] = -INFINITY;
  }
#pragma unroll
  for (int j = 0; j < Q; ++j) sxv[j] = 0;
#pragma unroll 2
  for (int64_t e = lo + lane; e < hi; e += 64) {
    const int64_t cell = gcell[e];
    const double x = (double)gval[e];
    const uint32_t m = mask[cell];
    if (m == 0) continue;
    double v[Q];
    const double* row = tab + cell * Q;
#pragma unroll
    for (int j = 0; j < Q; ++j) v[j] = row[j];
    if (SHARED) {
      sx[0] += x;
      sxx[0] = fma(x, x, sxx[0]);
      mn[0] = fmin(mn[0], x);
      mx[0] = fmax(mx[0], x);
      cnt[0] += 1.0;
#pragma unroll
      for (int j = 0; j < Q; ++j) sxv[j] = fma(x, v[j], sxv[j]);
    } else {
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        if (m >> j & 1) {
          sx[j] += x;
          sxx[j] = fma(x, x, sxx[j]);
          mn[j] = fmin(mn[j], x);
          mx[j] = fmax(mx[j], x);
          cnt[j] += 1.0;
          sxv[j] = fma(x, v[j], sxv[j]);
        }
      }
    }
  }
  double* o = part + ch * F;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const double a = wave_sum(sx[s]), b = wave_sum(sxx[s]), c0 = wave_min_any(mn[s]), c1 = wave_max_any(mx[s]),
                 d = wave_sum(cnt[s]);
    if (lane == 0) {
      o[s] = a; o[S + s] = b; o[2 * S + s] = c0; o[3 * S + s] = c1; o[4 * S + s] = d;
    }
  }
#pragma unroll
  for (int j = 0; j < Q; ++j) {
    const double a = wave_sum(sxv[j]);
    if (lane == 0) o[5 * S + j] = a;
  }
}

__global__ __launch_bounds__(256) void k_gc_finish_sparse(const double* __restrict__ part, const int64_t* __restrict__ gchunk,
                                                          int64_t G, int q, int Q, int S, const double* __restrict__ ks,
                                                          double* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int F = 5 * S + Q;
  const int64_t c0 = gchunk[g], c1 = gchunk[g + 1];
  double sx = 0, sxx = 0, mn = INFINITY, mx = -INFINITY, cnt = 0;
  for (int j = 0; j < q; ++j) {
    const int s = S == 1 ? 0 : j;
    if (j == 0 || S != 1) {
      sx = 0; sxx = 0; mn = INFINITY; mx = -INFINITY; cnt = 0;
      for (int64_t ch = c0; ch < c1; ++ch) {     // chunk order: the order of the cells
        const double* o = part + ch * F;
        sx += o[s];
        sxx += o[S + s];
        mn = fmin(mn, o[2 * S + s]);
        mx = fmax(mx, o[3 * S + s]);
        cnt += o[4 * S + s];
      }
    }
    double sxv = 0;
    for (int64_t ch = c0; ch < c1; ++ch) sxv += part[ch * F + 5 * S + j];
    out[(int64_t)j * G + g] = gc_r(sx, sxx, mn, mx, cnt, sxv, ks + j * KS_LD);
  }
}

// ------------------------------------------------------------------ upload helpers
// indices as the caller stores them (4 or 8 bytes) -> int32, checked against [0, limit); offsets -> int64
// (src may be dst when the indices already take 4 bytes: the pass then only checks)
__global__ __launch_bounds__(256) void k_narrow_idx(const void* src, int index_bytes, int64_t count, int64_t limit, int32_t* dst,
                                                    int* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const int64_t v = index_bytes == 8 ? static_cast<const int64_t*>(src)[i] : (int64_t) static_cast<const int32_t*>(src)[i];
    if (v < 0 || v >= limit) {
      atomicOr(bad, 1);
      dst[i] = 0;
    } else {
      dst[i] = (int32_t)v;
    }
  }
}

// CSR -> gene-major, stable in the cell index.  The cells are cut into B blocks of rows_per_block rows:
//   k_tr_count  cnt[b][g] = entries of gene g in block b (integer atomics)
//   k_tr_scan   per gene: cnt[b][g] -> entries of g in the blocks before b; total[g]
//   k_tr_fill   one workgroup per block walks its rows IN ORDER (a barrier between two rows): an entry of gene g goes to
//               gptr[g] + cursor[b][g]++.  A row names a gene once (canonical input), so within a gene the cells ascend.
__global__ __launch_bounds__(256) void k_tr_count(const int64_t* __restrict__ rptr, const int32_t* __restrict__ ridx, int64_t n,
                                                  int64_t G, int64_t rows_per_block, unsigned int* __restrict__ cnt) {
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  if (r0 >= r1) return;
  unsigned int* mine = cnt + (int64_t)blockIdx.x * G;
  for (int64_t e = rptr[r0] + threadIdx.x; e < rptr[r1]; e += blockDim.x) atomicAdd(mine + ridx[e], 1u);
}

__global__ __launch_bounds__(256) void k_tr_scan(unsigned int* __restrict__ cnt, int64_t G, int B, int64_t* __restrict__ total) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  int64_t run = 0;
  for (int b = 0; b < B; ++b) {
    const unsigned int t = cnt[(int64_t)b * G + g];
    cnt[(int64_t)b * G + g] = (unsigned int)run;
    run += t;
  }
  total[g] = run;
}

template <typename T>
__global__ __launch_bounds__(256) void k_tr_fill(const int64_t* __restrict__ rptr, const int32_t* __restrict__ ridx,
                                                 const T* __restrict__ rval, int64_t n, int64_t G, int64_t rows_per_block,
                                                 unsigned int* __restrict__ cnt, const int64_t* __restrict__ gptr,
                                                 int32_t* __restrict__ gcell, T* __restrict__ gval) {
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  unsigned int* mine = cnt + (int64_t)blockIdx.x * G;
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t lo = rptr[r], hi = rptr[r + 1];
    for (int64_t e = lo + threadIdx.x; e < hi; e += blockDim.x) {
      const int32_t g = ridx[e];
      const int64_t pos = gptr[g] + (int64_t)atomicAdd(mine + g, 1u);
      gcell[pos] = (int32_t)r;
      gval[pos] = rval[e];
    }
    __syncthreads();
  }
}

// offsets the caller stores in 4 or 8 bytes -> int64 on the host, checked: start at 0, never fall, end at nnz
bool widen_offsets(const void* p, int index_bytes, int64_t count, int64_t nnz, std::vector<int64_t>& out) {
  out.resize((size_t)count);
  for (int64_t i = 0; i < count; ++i)
    out[(size_t)i] = index_bytes == 8 ? static_cast<const int64_t*>(p)[i] : (int64_t) static_cast<const int32_t*>(p)[i];
  if (out[0] != 0 || out[(size_t)count - 1] != nnz) return false;
  for (int64_t i = 1; i < count; ++i)
    if (out[(size_t)i] < out[(size_t)i - 1]) return false;
  return true;
}

// chunks of the gene lists (Appendix B's split rule: a list longer than a chunk is cut into fixed chunks summed by
// separate waves, the partials are added in chunk order)
int build_chunks(cna_ctx* c, ExprState* s, const std::vector<int64_t>& gptr) {
  const int64_t waves = 256 * 16;
  int64_t len = s->nnz / (waves * 4);
  len = std::max<int64_t>(1024, std::min<int64_t>(65536, len));
  len = (len + 63) / 64 * 64;
  std::vector<int64_t> lo, first((size_t)s->G + 1);
  std::vector<int32_t> gene;
  for (int64_t g = 0; g < s->G; ++g) {
    first[(size_t)g] = (int64_t)lo.size();
    for (int64_t e = gptr[(size_t)g]; e < gptr[(size_t)g + 1]; e += len) {
      lo.push_back(e);
      gene.push_back((int32_t)g);
    }
  }
  first[(size_t)s->G] = (int64_t)lo.size();
  s->gchunk_h = first;
  s->nchunks = (int64_t)lo.size();
  s->chunk_len = len;
  CNA_TRY(buf_need(c, s, s->chunk_lo, 8 * std::max<int64_t>(1, s->nchunks)));
  CNA_TRY(buf_need(c, s, s->chunk_gene, 4 * std::max<int64_t>(1, s->nchunks)));
  CNA_TRY(buf_need(c, s, s->gchunk, 8 * (s->G + 1)));
  if (s->nchunks) {
    HIP_TRY(hipMemcpyAsync(s->chunk_lo.p, lo.data(), 8 * (size_t)s->nchunks, hipMemcpyHostToDevice, s->st));
    HIP_TRY(hipMemcpyAsync(s->chunk_gene.p, gene.data(), 4 * (size_t)s->nchunks, hipMemcpyHostToDevice, s->st));
  }
  HIP_TRY(hipMemcpyAsync(s->gchunk.p, first.data(), 8 * (size_t)(s->G + 1), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  return 0;
}

int upload_sparse(cna_ctx* c, ExprState* s, const void* indptr, const void* indices, const void* data, int64_t n, int64_t G,
                  int64_t nnz, int index_bytes, int is_f64, int is_csc) {
  const int64_t vb = is_f64 ? 8 : 4;
  const int64_t nmajor = is_csc ? G : n;
  std::vector<int64_t> off;
  if (!widen_offsets(indptr, index_bytes, nmajor + 1, nnz, off))
    CNA_FAIL(CNA_EINVAL, "expression matrix: indptr must start at 0, never fall and end at nnz");
  s->n = n; s->G = G; s->nnz = nnz; s->is_f64 = is_f64;
  Buf raw_idx, raw_val, rptr, ridx, cnt, total, bad;
  int rc = 0;
  auto cleanup = [&]() {
    (void)hipStreamSynchronize(s->st);
    for (Buf* b : {&raw_idx, &raw_val, &rptr, &ridx, &cnt, &total, &bad}) buf_free(c, *b);
  };
#define UP_TRY(expr)                 \
  do {                               \
    rc = (expr);                     \
    if (rc != 0) {                   \
      cleanup();                     \
      return rc;                     \
    }                                \
  } while (0)
#define UP_HIP(expr)                                                                  \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess) {                                                           \
      cna_set_error(std::string(#expr) + ": " + hipGetErrorString(_e));               \
      cleanup();                                                                      \
      return (int)_e;                                                                 \
    }                                                                                 \
  } while (0)
  const int64_t nz1 = std::max<int64_t>(1, nnz);
  const unsigned grid_e = (unsigned)std::min<int64_t>((nz1 + 255) / 256, 1 << 20);
  UP_TRY(buf_need(c, s, bad, 256));
  UP_HIP(hipMemsetAsync(bad.p, 0, 4, s->st));
  UP_TRY(buf_need(c, s, s->gptr, 8 * (G + 1)));
  UP_TRY(buf_need(c, s, s->gcell, 4 * nz1));
  UP_TRY(buf_need(c, s, s->gval, vb * nz1));
  std::vector<int64_t> gptr_h;
  int bad_h = 0;
  if (is_csc) {
    // gene-major already: the cell of every entry, narrowed to 4 bytes and checked on the device
    if (index_bytes == 8) {
      UP_TRY(buf_need(c, s, raw_idx, 8 * nz1));
      UP_HIP(hipMemcpyAsync(raw_idx.p, indices, 8 * (size_t)nnz, hipMemcpyHostToDevice, s->st));
      hipLaunchKernelGGL(k_narrow_idx, dim3(grid_e), dim3(256), 0, s->st, raw_idx.p, 8, nnz, n, (int32_t*)s->gcell.p, (int*)bad.p);
    } else {
      UP_HIP(hipMemcpyAsync(s->gcell.p, indices, 4 * (size_t)nnz, hipMemcpyHostToDevice, s->st));
      hipLaunchKernelGGL(k_narrow_idx, dim3(grid_e), dim3(256), 0, s->st, s->gcell.p, 4, nnz, n, (int32_t*)s->gcell.p, (int*)bad.p);
    }
    UP_HIP(hipGetLastError());
    UP_HIP(hipMemcpyAsync(s->gval.p, data, (size_t)(vb * nnz), hipMemcpyHostToDevice, s->st));
    UP_HIP(hipMemcpyAsync(&bad_h, bad.p, 4, hipMemcpyDeviceToHost, s->st));
    UP_HIP(hipStreamSynchronize(s->st));
    if (bad_h) {
      cleanup();
      CNA_FAIL(CNA_EINVAL, "expression matrix: a row index lies outside [0, n_cells)");
    }
    gptr_h = off;
  } else {
    // the transpose needs the rows' indices and values beside the gene-major copy for a moment
    UP_TRY(buf_need(c, s, rptr, 8 * (n + 1)));
    UP_TRY(buf_need(c, s, ridx, 4 * nz1));
    UP_TRY(buf_need(c, s, raw_val, vb * nz1));
    UP_HIP(hipMemcpyAsync(rptr.p, off.data(), 8 * (size_t)(n + 1), hipMemcpyHostToDevice, s->st));
    if (index_bytes == 8) {
      UP_TRY(buf_need(c, s, raw_idx, 8 * nz1));
      UP_HIP(hipMemcpyAsync(raw_idx.p, indices, 8 * (size_t)nnz, hipMemcpyHostToDevice, s->st));
      hipLaunchKernelGGL(k_narrow_idx, dim3(grid_e), dim3(256), 0, s->st, raw_idx.p, 8, nnz, G, (int32_t*)ridx.p, (int*)bad.p);
    } else {
      UP_HIP(hipMemcpyAsync(ridx.p, indices, 4 * (size_t)nnz, hipMemcpyHostToDevice, s->st));
      hipLaunchKernelGGL(k_narrow_idx, dim3(grid_e), dim3(256), 0, s->st, ridx.p, 4, nnz, G, (int32_t*)ridx.p, (int*)bad.p);
    }
    UP_HIP(hipGetLastError());
    UP_HIP(hipMemcpyAsync(raw_val.p, data, (size_t)(vb * nnz), hipMemcpyHostToDevice, s->st));
    UP_HIP(hipMemcpyAsync(&bad_h, bad.p, 4, hipMemcpyDeviceToHost, s->st));
    UP_HIP(hipStreamSynchronize(s->st));
    if (bad_h) {
      cleanup();
      CNA_FAIL(CNA_EINVAL, "expression matrix: a column index lies outside [0, n_genes)");
    }
    if (raw_idx.p) buf_free(c, raw_idx);
    // blocks of rows: at most 2048, and a counter table of at most 64M words
    int64_t B = std::min<int64_t>(2048, std::max<int64_t>(1, (64ll << 20) / G));
    B = std::min<int64_t>(B, n);
    const int64_t rpb = (n + B - 1) / B;
    B = (n + rpb - 1) / rpb;
    UP_TRY(buf_need(c, s, cnt, 4 * B * G));
    UP_TRY(buf_need(c, s, total, 8 * G));
    UP_HIP(hipMemsetAsync(cnt.p, 0, (size_t)(4 * B * G), s->st));
    hipLaunchKernelGGL(k_tr_count, dim3((unsigned)B), dim3(256), 0, s->st, (const int64_t*)rptr.p, (const int32_t*)ridx.p, n, G,
                       rpb, (unsigned int*)cnt.p);
    hipLaunchKernelGGL(k_tr_scan, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s->st, (unsigned int*)cnt.p, G, (int)B,
                       (int64_t*)total.p);
    UP_HIP(hipGetLastError());
    std::vector<int64_t> tot((size_t)G);
    UP_HIP(hipMemcpyAsync(tot.data(), total.p, 8 * (size_t)G, hipMemcpyDeviceToHost, s->st));
    UP_HIP(hipStreamSynchronize(s->st));
    gptr_h.assign((size_t)G + 1, 0);
    for (int64_t g = 0; g < G; ++g) gptr_h[(size_t)g + 1] = gptr_h[(size_t)g] + tot[(size_t)g];
    if (gptr_h[(size_t)G] != nnz) {
      cleanup();
      CNA_FAIL(CNA_EINVAL, "expression matrix: the transpose lost entries (internal error)");
    }
    UP_HIP(hipMemcpyAsync(s->gptr.p, gptr_h.data(), 8 * (size_t)(G + 1), hipMemcpyHostToDevice, s->st));
    if (is_f64)
      hipLaunchKernelGGL(k_tr_fill<double>, dim3((unsigned)B), dim3(256), 0, s->st, (const int64_t*)rptr.p, (const int32_t*)ridx.p,
                         (const double*)raw_val.p, n, G, rpb, (unsigned int*)cnt.p, (const int64_t*)s->gptr.p,
                         (int32_t*)s->gcell.p, (double*)s->gval.p);
    else
      hipLaunchKernelGGL(k_tr_fill<float>, dim3((unsigned)B), dim3(256), 0, s->st, (const int64_t*)rptr.p, (const int32_t*)ridx.p,
                         (const float*)raw_val.p, n, G, rpb, (unsigned int*)cnt.p, (const int64_t*)s->gptr.p,
                         (int32_t*)s->gcell.p, (float*)s->gval.p);
    UP_HIP(hipGetLastError());
    UP_HIP(hipStreamSynchronize(s->st));
  }
  if (is_csc) UP_HIP(hipMemcpyAsync(s->gptr.p, gptr_h.data(), 8 * (size_t)(G + 1), hipMemcpyHostToDevice, s->st));
  cleanup();
  CNA_TRY(build_chunks(c, s, gptr_h));
  return 0;
#undef UP_TRY
#undef UP_HIP
}

template <typename T, int Q>
int launch_dense_q(ExprState* s, bool shared, int nslab, int64_t slab_rows) {
  const dim3 grid((unsigned)((s->G + 63) / 64), (unsigned)nslab);
  if (shared)
    hipLaunchKernelGGL((k_gc_dense<T, Q, true>), grid, dim3(64), 0, s->st, (const T*)s->X.p, s->n, s->G, slab_rows,
                       (const double*)s->vtab.p, (const uint32_t*)s->vmask.p, (double*)s->part.p);
  else
    hipLaunchKernelGGL((k_gc_dense<T, Q, false>), grid, dim3(64), 0, s->st, (const T*)s->X.p, s->n, s->G, slab_rows,
                       (const double*)s->vtab.p, (const uint32_t*)s->vmask.p, (double*)s->part.p);
  return 0;
}

template <typename T, int Q>
int launch_sparse_q(ExprState* s, bool shared) {
  const dim3 grid((unsigned)((s->nchunks + 3) / 4));
  if (shared)
    hipLaunchKernelGGL((k_gc_sparse<T, Q, true>), grid, dim3(256), 0, s->st, (const int64_t*)s->chunk_lo.p,
                       (const int32_t*)s->chunk_gene.p, (const int64_t*)s->gptr.p, s->nchunks, s->chunk_len,
                       (const int32_t*)s->gcell.p, (const T*)s->gval.p, (const double*)s->vtab.p, (const uint32_t*)s->vmask.p,
                       (double*)s->part.p);
  else
    hipLaunchKernelGGL((k_gc_sparse<T, Q, false>), grid, dim3(256), 0, s->st, (const int64_t*)s->chunk_lo.p,
                       (const int32_t*)s->chunk_gene.p, (const int64_t*)s->gptr.p, s->nchunks, s->chunk_len,
                       (const int32_t*)s->gcell.p, (const T*)s->gval.p, (const double*)s->vtab.p, (const uint32_t*)s->vmask.p,
                       (double*)s->part.p);
  return 0;
}

template <typename T>
int launch_pass(ExprState* s, int Q, bool shared, int nslab, int64_t slab_rows) {
  const bool dense = s->format == 1;
  switch (Q) {
    case 1: return dense ? launch_dense_q<T, 1>(s, shared, nslab, slab_rows) : launch_sparse_q<T, 1>(s, shared);
    case 2: return dense ? launch_dense_q<T, 2>(s, shared, nslab, slab_rows) : launch_sparse_q<T, 2>(s, shared);
    case 4: return dense ? launch_dense_q<T, 4>(s, shared, nslab, slab_rows) : launch_sparse_q<T, 4>(s, shared);
    case 8: return dense ? launch_dense_q<T, 8>(s, shared, nslab, slab_rows) : launch_sparse_q<T, 8>(s, shared);
    default: return dense ? launch_dense_q<T, 16>(s, shared, nslab, slab_rows) : launch_sparse_q<T, 16>(s, shared);
  }
}

// ------------------------------------------------------------------ per-bin sums (cna_expr_to_bins)
constexpr int PB_MAX_BINS = 4096;
constexpr int64_t PB_DENSE_CHUNK = 2048;          // cells of one bin that one workgroup of k_pb_dense adds up
constexpr int64_t PB_PART_BYTES = 256ll << 20;    // partial sums of the gene-major kernel kept at a time
constexpr int PB_MAX_BLOCKS = 1024;               // blocks of cells of the counting sort

// block b: cnt[b][bin] = cells of [r0, r1) with that code; *bad |= 1 for a code outside [-1, n_bins)
__global__ __launch_bounds__(256) void k_pb_count(const int32_t* __restrict__ codes, int64_t n, int n_bins, int64_t rows_per_block,
                                                  unsigned int* __restrict__ cnt, int* __restrict__ bad) {
  __shared__ unsigned int h[PB_MAX_BINS];
  for (int b = threadIdx.x; b < n_bins; b += blockDim.x) h[b] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  for (int64_t i = r0 + threadIdx.x; i < r1; i += blockDim.x) {
    const int32_t cd = codes[i];
    if (cd < -1 || cd >= n_bins) atomicOr(bad, 1);
    else if (cd >= 0) atomicAdd(&h[cd], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < n_bins; b += blockDim.x) cnt[(int64_t)blockIdx.x * n_bins + b] = h[b];
}

// one wave per block of cells; cur[bin] = cells of the bin in the blocks before this one plus those already placed.  Among
// the 64 cells of a batch equal codes are ranked by lane, so a bin's cells ascend.
__global__ __launch_bounds__(64) void k_pb_fill(const int32_t* __restrict__ codes, int64_t n, int n_bins, int64_t rows_per_block,
                                                const unsigned int* __restrict__ cnt, const int64_t* __restrict__ bptr,
                                                int32_t* __restrict__ list) {
  __shared__ unsigned int cur[PB_MAX_BINS];
  const int lane = threadIdx.x;
  for (int b = lane; b < n_bins; b += 64) cur[b] = cnt[(int64_t)blockIdx.x * n_bins + b];
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  for (int64_t base = r0; base < r1; base += 64) {
    const int64_t i = base + lane;
    const int32_t cd = i < r1 ? codes[i] : -1;
    unsigned int rank = 0;
    bool last = true;
    for (int j = 0; j < 64; ++j) {
      const bool same = __shfl(cd, j, 64) == cd;
      rank += (same && j < lane) ? 1u : 0u;
      last = last && !(same && j > lane);
    }
    if (cd >= 0) list[bptr[cd] + (int64_t)(cur[cd] + rank)] = (int32_t)i;
    __syncthreads();
    if (cd >= 0 && last) cur[cd] += rank + 1u;
    __syncthreads();
  }
}

// grid.x = chunk * gene_blocks + gene block (neighbouring workgroups read neighbouring pieces of the same rows);
// rng[2 ch], rng[2 ch + 1]: the chunk's span of the cell list (never empty).  COUNT: add 1 where x > 0 instead of x.
template <typename T, bool COUNT>
__global__ __launch_bounds__(256) void k_pb_dense(const T* __restrict__ X, int64_t G, int64_t gene_blocks,
                                                  const int32_t* __restrict__ list, const int64_t* __restrict__ rng,
                                                  double* __restrict__ part) {
  constexpr int U = 8;
  const int64_t ch = (int64_t)blockIdx.x / gene_blocks, gb = (int64_t)blockIdx.x % gene_blocks;
  const int64_t g = gb * blockDim.x + threadIdx.x;
  const bool act = g < G;
  const int64_t gl = act ? g : G - 1;          // idle lanes of the last gene block reload its last gene; nothing is stored
  const int64_t lo = rng[2 * ch], hi = rng[2 * ch + 1];
  double acc = 0.0;
  for (int64_t e = lo; e < hi; e += U) {
    T xs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ee = e + u < hi ? e + u : hi - 1;
      xs[u] = X[(int64_t)list[ee] * G + gl];   // list[ee] is the same in every lane: a scalar load
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (e + u >= hi) break;
      acc += COUNT ? (xs[u] > (T)0 ? 1.0 : 0.0) : (double)xs[u];
    }
  }
  if (act) part[ch * G + g] = acc;
}

// out[bin][gene] = the bin's partials added in chunk order (bfirst: first chunk of every bin, n_bins + 1 entries)
__global__ __launch_bounds__(256) void k_pb_finish_dense(const double* __restrict__ part, int64_t G, int n_bins,
                                                         const int64_t* __restrict__ bfirst, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)n_bins * G) return;
  const int64_t b = t / G, g = t % G;
  double s = 0.0;
  for (int64_t ch = bfirst[b]; ch < bfirst[b + 1]; ++ch) s += part[ch * G + g];
  out[t] = s;
}

// one wave per chunk c0 + blockIdx.x of the gene lists; dynamic LDS: n_bins doubles (the sums) and n_bins ints (turns).
// A batch is 64 consecutive entries.  Where every lane of a batch that takes part names the same bin, the wave adds them
// by its fixed tree and lane 0 adds the total; otherwise rounds: every waiting lane posts stamp * 64 + 63 - lane with an
// integer atomic max, the lowest waiting lane of each bin finds its own value there and adds.  Both orders depend on the
// input alone.
template <typename T, bool COUNT>
__global__ __launch_bounds__(64) void k_pb_sparse(const int64_t* __restrict__ chunk_lo, const int32_t* __restrict__ chunk_gene,
                                                  const int64_t* __restrict__ gptr, int64_t c0, int64_t chunk_len,
                                                  const int32_t* __restrict__ gcell, const T* __restrict__ gval,
                                                  const int32_t* __restrict__ codes, int n_bins, double* __restrict__ part) {
  extern __shared__ double pb_lds[];
  double* acc = pb_lds;
  int* turn = reinterpret_cast<int*>(pb_lds + n_bins);
  const int lane = threadIdx.x;
  const int64_t ch = c0 + blockIdx.x;
  for (int b = lane; b < n_bins; b += 64) {
    acc[b] = 0.0;
    turn[b] = 0;
  }
  __syncthreads();
  const int64_t lo = chunk_lo[ch];
  const int64_t end = gptr[chunk_gene[ch] + 1];
  const int64_t hi = lo + chunk_len < end ? lo + chunk_len : end;
  int stamp = 0;
  for (int64_t e0 = lo; e0 < hi; e0 += 64) {
    const int64_t e = e0 + lane;
    int32_t bin = -1;
    double v = 0.0;
    if (e < hi) {
      bin = codes[gcell[e]];
      const T x = gval[e];
      v = COUNT ? (x > (T)0 ? 1.0 : 0.0) : (double)x;
    }
    bool wait = bin >= 0;
    const unsigned long long in = __ballot(wait);
    if (in == 0) continue;
    const int32_t b0 = __shfl(bin, __ffsll((long long)in) - 1, 64);
    if (__ballot(wait && bin != b0) == 0) {
      const double s = wave_sum(wait ? v : 0.0);
      if (lane == 0) acc[b0] += s;
      __syncthreads();
      continue;
    }
    while (true) {
      ++stamp;
      const int mine = stamp * 64 + 63 - lane;
      if (wait) atomicMax(&turn[bin], mine);
      __syncthreads();
      if (wait && turn[bin] == mine) {
        acc[bin] += v;
        wait = false;
      }
      __syncthreads();
      if (__ballot(wait) == 0) break;
    }
  }
  __syncthreads();
  double* o = part + (int64_t)blockIdx.x * n_bins;
  for (int b = lane; b < n_bins; b += 64) o[b] = acc[b];
}

// genes [g0, g1) of a tile whose first chunk is c0: out[bin][gene] = the gene's partials added in chunk order
__global__ __launch_bounds__(256) void k_pb_finish_sparse(const double* __restrict__ part, const int64_t* __restrict__ gchunk,
                                                          int64_t g0, int64_t g1, int64_t c0, int n_bins, int64_t G,
                                                          double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (g1 - g0) * n_bins) return;
  const int64_t g = g0 + t / n_bins, b = t % n_bins;
  double s = 0.0;
  for (int64_t ch = gchunk[g]; ch < gchunk[g + 1]; ++ch) s += part[(ch - c0) * n_bins + b];
  out[b * G + g] = s;
}

template <typename T>
int pb_dense(cna_ctx* c, ExprState* s, int n_bins, bool count, const std::vector<int64_t>& tot) {
  const int64_t n = s->n, G = s->G;
  std::vector<int64_t> bptr((size_t)n_bins + 1, 0), first((size_t)n_bins + 1, 0), rng;
  for (int b = 0; b < n_bins; ++b) {
    bptr[(size_t)b + 1] = bptr[(size_t)b] + tot[(size_t)b];
    first[(size_t)b] = (int64_t)rng.size() / 2;
    for (int64_t e = bptr[(size_t)b]; e < bptr[(size_t)b + 1]; e += PB_DENSE_CHUNK) {
      rng.push_back(e);
      rng.push_back(std::min(e + PB_DENSE_CHUNK, bptr[(size_t)b + 1]));
    }
  }
  const int64_t nch = (int64_t)rng.size() / 2;
  first[(size_t)n_bins] = nch;
  const int threads = (int)std::min<int64_t>(256, (G + 63) / 64 * 64);
  const int64_t gene_blocks = (G + threads - 1) / threads;
  if (nch * gene_blocks > 0x7fffffffll) CNA_FAIL(CNA_EINVAL, "cna_expr_to_bins: more than 2^31 - 1 workgroups (chunks x gene blocks)");
  CNA_TRY(buf_need(c, s, s->blist, 4 * n));
  CNA_TRY(buf_need(c, s, s->bptr, 8 * ((int64_t)n_bins + 1)));
  CNA_TRY(buf_need(c, s, s->bfirst, 8 * ((int64_t)n_bins + 1)));
  CNA_TRY(buf_need(c, s, s->brng, 16 * std::max<int64_t>(1, nch)));
  CNA_TRY(buf_need(c, s, s->part, 8 * std::max<int64_t>(1, nch) * G));
  HIP_TRY(hipMemcpyAsync(s->bptr.p, bptr.data(), 8 * bptr.size(), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipMemcpyAsync(s->bfirst.p, first.data(), 8 * first.size(), hipMemcpyHostToDevice, s->st));
  if (nch) HIP_TRY(hipMemcpyAsync(s->brng.p, rng.data(), 8 * rng.size(), hipMemcpyHostToDevice, s->st));
  const int64_t rpb = round_up64((n + PB_MAX_BLOCKS - 1) / PB_MAX_BLOCKS, 64);
  const unsigned B = (unsigned)((n + rpb - 1) / rpb);
  hipLaunchKernelGGL(k_pb_fill, dim3(B), dim3(64), 0, s->st, (const int32_t*)s->bcode.p, n, n_bins, rpb,
                     (const unsigned int*)s->bcnt.p, (const int64_t*)s->bptr.p, (int32_t*)s->blist.p);
  if (nch) {
    const dim3 grid((unsigned)(nch * gene_blocks));
    if (count)
      hipLaunchKernelGGL((k_pb_dense<T, true>), grid, dim3(threads), 0, s->st, (const T*)s->X.p, G, gene_blocks,
                         (const int32_t*)s->blist.p, (const int64_t*)s->brng.p, (double*)s->part.p);
    else
      hipLaunchKernelGGL((k_pb_dense<T, false>), grid, dim3(threads), 0, s->st, (const T*)s->X.p, G, gene_blocks,
                         (const int32_t*)s->blist.p, (const int64_t*)s->brng.p, (double*)s->part.p);
  }
  hipLaunchKernelGGL(k_pb_finish_dense, dim3((unsigned)(((int64_t)n_bins * G + 255) / 256)), dim3(256), 0, s->st,
                     (const double*)s->part.p, G, n_bins, (const int64_t*)s->bfirst.p, (double*)s->rout.p);
  HIP_TRY(hipGetLastError());
  return 0;
}

template <typename T>
int pb_sparse(cna_ctx* c, ExprState* s, int n_bins, bool count) {
  const int64_t G = s->G;
  const int64_t max_chunks = std::max<int64_t>(1, PB_PART_BYTES / (8 * (int64_t)n_bins));
  const std::vector<int64_t>& gc = s->gchunk_h;
  // tiles of whole genes, each with at most max_chunks chunks (one gene at least)
  int64_t need = 1;
  for (int64_t g0 = 0; g0 < G;) {
    int64_t g1 = g0 + 1;
    while (g1 < G && gc[(size_t)g1 + 1] - gc[(size_t)g0] <= max_chunks) ++g1;
    need = std::max(need, gc[(size_t)g1] - gc[(size_t)g0]);
    g0 = g1;
  }
  if (need > 0x7fffffffll / 256) CNA_FAIL(CNA_EINVAL, "cna_expr_to_bins: one gene has too many chunks");
  CNA_TRY(buf_need(c, s, s->part, 8 * need * n_bins));
  const size_t lds = (size_t)n_bins * 12;
  for (int64_t g0 = 0; g0 < G;) {
    int64_t g1 = g0 + 1;
    while (g1 < G && gc[(size_t)g1 + 1] - gc[(size_t)g0] <= max_chunks) ++g1;
    const int64_t c0 = gc[(size_t)g0], nch = gc[(size_t)g1] - c0;
    if (nch) {
      if (count)
        hipLaunchKernelGGL((k_pb_sparse<T, true>), dim3((unsigned)nch), dim3(64), lds, s->st, (const int64_t*)s->chunk_lo.p,
                           (const int32_t*)s->chunk_gene.p, (const int64_t*)s->gptr.p, c0, s->chunk_len,
                           (const int32_t*)s->gcell.p, (const T*)s->gval.p, (const int32_t*)s->bcode.p, n_bins,
                           (double*)s->part.p);
      else
        hipLaunchKernelGGL((k_pb_sparse<T, false>), dim3((unsigned)nch), dim3(64), lds, s->st, (const int64_t*)s->chunk_lo.p,
                           (const int32_t*)s->chunk_gene.p, (const int64_t*)s->gptr.p, c0, s->chunk_len,
                           (const int32_t*)s->gcell.p, (const T*)s->gval.p, (const int32_t*)s->bcode.p, n_bins,
                           (double*)s->part.p);
    }
    hipLaunchKernelGGL(k_pb_finish_sparse, dim3((unsigned)(((g1 - g0) * n_bins + 255) / 256)), dim3(256), 0, s->st,
                       (const double*)s->part.p, (const int64_t*)s->gchunk.p, g0, g1, c0, n_bins, G, (double*)s->rout.p);
    g0 = g1;
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ expression x working matrix (cna_expr_cross)
constexpr int XC_TS = 32;             // samples per tile of k_xc_dense: 64 accumulator registers per lane
constexpr int XC_MAX_COLS = 1024;
constexpr int64_t XC_PART_BYTES = 1ll << 30;   // partial sums of the dense kernel at most

// *bad |= 1: a value outside [-1, nx); |= 2: an X row named twice.  *m += cells that take part.
__global__ __launch_bounds__(256) void k_xc_check(const int64_t* __restrict__ xrow, int64_t n, int64_t nx,
                                                  unsigned int* __restrict__ seen, int* __restrict__ bad,
                                                  unsigned long long* __restrict__ m) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long mine = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t v = xrow[i];
    if (v < -1 || v >= nx) {
      atomicOr(bad, 1);
    } else if (v >= 0) {
      if (atomicAdd(seen + v, 1u) != 0u) atomicOr(bad, 2);
      ++mine;
    }
  }
  if (mine) atomicAdd(m, mine);
}

// the cells [r0, r1) of a slab against the samples [s0, s0 + ns) of X; FULL: ns == XC_TS (no index is clamped)
template <typename T, bool FULL>
__device__ __forceinline__ void xc_slab(const T* __restrict__ E, int64_t G, int64_t gl, int64_t r0, int64_t r1,
                                        const int64_t* __restrict__ xrow, const double* __restrict__ Xw, int ldx, int s0,
                                        int ns, bool first, double* acc, double& sx, double& sxx) {
  constexpr int U = 4;
  for (int64_t r = r0; r < r1; r += U) {
    T xs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t rr = r + u < r1 ? r + u : r1 - 1;
      xs[u] = E[rr * G + gl];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (r + u >= r1) break;
      const int64_t xr = xrow[r + u];          // wave-uniform: a scalar load and a scalar branch
      if (xr < 0) continue;
      const double* v = Xw + xr * ldx + s0;    // ... and so is the row of X: scalar loads, one uniform operand per FMA
      const double x = (double)xs[u];
      if (first) {
        sx += x;
        sxx = fma(x, x, sxx);
      }
#pragma unroll
      for (int s = 0; s < XC_TS; ++s) acc[s] = fma(x, v[FULL ? s : (s < ns ? s : ns - 1)], acc[s]);
    }
  }
}

// grid.x = gene block * ntile + tile (the tiles of one slab of E run side by side: its rows come from the cache for all
// but the first), grid.y = slab.  part[(slab * Nx + s) * G + g], part2[(slab * 2 + {0: sum x, 1: sum x^2}) * G + g]
template <typename T>
__global__ __launch_bounds__(64) void k_xc_dense(const T* __restrict__ E, int64_t n, int64_t G, int64_t slab_rows,
                                                 const int64_t* __restrict__ xrow, const double* __restrict__ Xw, int ldx,
                                                 int Nx, int ntile, double* __restrict__ part, double* __restrict__ part2) {
  const int tile = (int)(blockIdx.x % (unsigned)ntile);
  const int64_t g = (int64_t)(blockIdx.x / (unsigned)ntile) * 64 + threadIdx.x;
  const bool act = g < G;
  const int64_t gl = act ? g : G - 1;          // idle lanes of the last gene block reload its last gene; nothing is stored
  const int64_t r0 = (int64_t)blockIdx.y * slab_rows;
  const int64_t r1 = r0 + slab_rows < n ? r0 + slab_rows : n;
  const int s0 = tile * XC_TS;
  const int ns = Nx - s0 < XC_TS ? Nx - s0 : XC_TS;
  const bool first = tile == 0;
  double acc[XC_TS];
#pragma unroll
  for (int s = 0; s < XC_TS; ++s) acc[s] = 0.0;
  double sx = 0.0, sxx = 0.0;
  if (ns == XC_TS) xc_slab<T, true>(E, G, gl, r0, r1, xrow, Xw, ldx, s0, ns, first, acc, sx, sxx);
  else xc_slab<T, false>(E, G, gl, r0, r1, xrow, Xw, ldx, s0, ns, first, acc, sx, sxx);
  if (!act) return;
  double* o = part + ((int64_t)blockIdx.y * Nx + s0) * G + g;
#pragma unroll
  for (int s = 0; s < XC_TS; ++s)
    if (s < ns) o[(int64_t)s * G] = acc[s];
  if (first) {
    part2[((int64_t)blockIdx.y * 2) * G + g] = sx;
    part2[((int64_t)blockIdx.y * 2 + 1) * G + g] = sxx;
  }
}

// W[g][s] = the partials of (g, s) added in slab order
__global__ __launch_bounds__(256) void k_xc_finish_dense(const double* __restrict__ part, int64_t G, int Nx, int nslab,
                                                         double* __restrict__ W) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= G * Nx) return;
  const int64_t s = t / G, g = t % G;
  double a = 0.0;
  for (int p = 0; p < nslab; ++p) a += part[((int64_t)p * Nx + s) * G + g];
  W[g * Nx + s] = a;
}

// out[j] = part[0][j] + part[1][j] + ... in that order (records of len doubles)
__global__ __launch_bounds__(256) void k_xc_fold(const double* __restrict__ part, int64_t len, int np, double* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= len) return;
  double a = 0.0;
  for (int p = 0; p < np; ++p) a += part[(int64_t)p * len + j];
  out[j] = a;
}

// block b: part[b][s] = sum over its cells, ascending, of X[xrow[cell]][s]; thread = sample (+ 256, ...)
__global__ __launch_bounds__(256) void k_xc_rho(const int64_t* __restrict__ xrow, int64_t n, int64_t rows_per_block,
                                                const double* __restrict__ Xw, int ldx, int Nx, double* __restrict__ part) {
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  double acc[XC_MAX_COLS / 256] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t xr = xrow[r];
    if (xr < 0) continue;
    const double* v = Xw + xr * ldx;
#pragma unroll
    for (int k = 0; k < XC_MAX_COLS / 256; ++k) {
      const int s = threadIdx.x + 256 * k;
      if (s < Nx) acc[k] += v[s];
    }
  }
#pragma unroll
  for (int k = 0; k < XC_MAX_COLS / 256; ++k) {
    const int s = threadIdx.x + 256 * k;
    if (s < Nx) part[(int64_t)blockIdx.x * Nx + s] = acc[k];
  }
}

__device__ __forceinline__ double lane_value(double v, int j) {   // lane j's value in every lane (j wave-uniform)
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

// one wave per chunk c0 + blockIdx.x of the gene lists; lane l holds the samples l, l + 64, ... (P of them).  The wave
// reads 64 entries at a time (cell -> X row, value) and takes them in order: the entries of a (gene, sample) are added
// in the order of the list.  part[blockIdx.x * Nx + s]; part2[2 ch], [2 ch + 1] = sum x, sum x^2 of the chunk's entries
// that take part.
template <typename T, int P>
__global__ __launch_bounds__(64) void k_xc_sparse(const int64_t* __restrict__ chunk_lo, const int32_t* __restrict__ chunk_gene,
                                                  const int64_t* __restrict__ gptr, int64_t c0, int64_t chunk_len,
                                                  const int32_t* __restrict__ gcell, const T* __restrict__ gval,
                                                  const int64_t* __restrict__ xrow, const double* __restrict__ Xw, int ldx,
                                                  int Nx, double* __restrict__ part, double* __restrict__ part2) {
  const int lane = threadIdx.x;
  const int64_t ch = c0 + blockIdx.x;
  const int64_t lo = chunk_lo[ch];
  const int64_t end = gptr[chunk_gene[ch] + 1];
  const int64_t hi = lo + chunk_len < end ? lo + chunk_len : end;
  double acc[P];
#pragma unroll
  for (int p = 0; p < P; ++p) acc[p] = 0.0;
  double sx = 0.0, sxx = 0.0;
  for (int64_t e0 = lo; e0 < hi; e0 += 64) {
    const int64_t e = e0 + lane;
    int xr = -1;                               // (rows of X < 2^31: the cells are)
    double x = 0.0;
    if (e < hi) {
      xr = (int)xrow[gcell[e]];
      x = (double)gval[e];
    }
    const int cnt = hi - e0 < 64 ? (int)(hi - e0) : 64;
    for (int j = 0; j < cnt; ++j) {
      const int xrj = __builtin_amdgcn_readlane(xr, j);
      if (xrj < 0) continue;
      const double xj = lane_value(x, j);
      const double* row = Xw + (int64_t)xrj * ldx;
      sx += xj;
      sxx = fma(xj, xj, sxx);
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int s = lane + 64 * p;
        if (s < Nx) acc[p] = fma(xj, row[s], acc[p]);
      }
    }
  }
  double* o = part + (int64_t)blockIdx.x * Nx;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int s = lane + 64 * p;
    if (s < Nx) o[s] = acc[p];
  }
  if (lane == 0) {
    part2[2 * ch] = sx;
    part2[2 * ch + 1] = sxx;
  }
}

// genes [g0, g1) of a tile whose first chunk is c0: W[g][s] = the gene's partials added in chunk order
__global__ __launch_bounds__(256) void k_xc_finish_sparse(const double* __restrict__ part, const int64_t* __restrict__ gchunk,
                                                          int64_t g0, int64_t g1, int64_t c0, int Nx, double* __restrict__ W) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (g1 - g0) * Nx) return;
  const int64_t g = g0 + t / Nx, s = t % Nx;
  double a = 0.0;
  for (int64_t ch = gchunk[g]; ch < gchunk[g + 1]; ++ch) a += part[(ch - c0) * Nx + s];
  W[g * Nx + s] = a;
}

__global__ __launch_bounds__(256) void k_xc_finish_sparse_sx(const double* __restrict__ part2, const int64_t* __restrict__ gchunk,
                                                             int64_t G, double* __restrict__ sx, double* __restrict__ sxx) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  double a = 0.0, b = 0.0;
  for (int64_t ch = gchunk[g]; ch < gchunk[g + 1]; ++ch) {
    a += part2[2 * ch];
    b += part2[2 * ch + 1];
  }
  sx[g] = a;
  sxx[g] = b;
}

template <typename T>
int xc_dense(cna_ctx* c, ExprState* s, const double* Xw, int ldx, int Nx, double* W, double* sx) {
  const int64_t n = s->n, G = s->G;
  const int ntile = (Nx + XC_TS - 1) / XC_TS;
  const int64_t gene_blocks = (G + 63) / 64;
  if (gene_blocks * ntile > 0x7fffffffll) CNA_FAIL(CNA_EINVAL, "cna_expr_cross: more than 2^31 - 1 workgroups (gene blocks x sample tiles)");
  // slabs: enough single-wave workgroups to fill the device, at least 128 cells each, partials held to XC_PART_BYTES
  int64_t nslab = std::min<int64_t>(2048, (8192 + gene_blocks * ntile - 1) / (gene_blocks * ntile));
  nslab = std::min<int64_t>(nslab, std::max<int64_t>(1, XC_PART_BYTES / (8 * (int64_t)Nx * G)));
  nslab = std::max<int64_t>(1, std::min<int64_t>(nslab, n / 128));
  const int64_t slab_rows = (n + nslab - 1) / nslab;
  nslab = (n + slab_rows - 1) / slab_rows;
  CNA_TRY(buf_need(c, s, s->xpart, 8 * nslab * Nx * G));
  CNA_TRY(buf_need(c, s, s->xpart2, 16 * nslab * G));
  hipLaunchKernelGGL((k_xc_dense<T>), dim3((unsigned)(gene_blocks * ntile), (unsigned)nslab), dim3(64), 0, s->st,
                     (const T*)s->X.p, n, G, slab_rows, (const int64_t*)s->xrow.p, Xw, ldx, Nx, ntile, (double*)s->xpart.p,
                     (double*)s->xpart2.p);
  hipLaunchKernelGGL(k_xc_finish_dense, dim3((unsigned)((G * Nx + 255) / 256)), dim3(256), 0, s->st, (const double*)s->xpart.p,
                     G, Nx, (int)nslab, W);
  hipLaunchKernelGGL(k_xc_fold, dim3((unsigned)((2 * G + 255) / 256)), dim3(256), 0, s->st, (const double*)s->xpart2.p, 2 * G,
                     (int)nslab, sx);
  HIP_TRY(hipGetLastError());
  return 0;
}

template <typename T, int P>
void xc_sparse_launch(ExprState* s, int64_t nch, int64_t c0, const double* Xw, int ldx, int Nx) {
  hipLaunchKernelGGL((k_xc_sparse<T, P>), dim3((unsigned)nch), dim3(64), 0, s->st, (const int64_t*)s->chunk_lo.p,
                     (const int32_t*)s->chunk_gene.p, (const int64_t*)s->gptr.p, c0, s->chunk_len, (const int32_t*)s->gcell.p,
                     (const T*)s->gval.p, (const int64_t*)s->xrow.p, Xw, ldx, Nx, (double*)s->xpart.p, (double*)s->xpart2.p);
}

template <typename T>
int xc_sparse(cna_ctx* c, ExprState* s, const double* Xw, int ldx, int Nx, double* W, double* sx) {
  const int64_t G = s->G;
  const int64_t max_chunks = std::max<int64_t>(1, PB_PART_BYTES / (8 * (int64_t)Nx));
  const std::vector<int64_t>& gc = s->gchunk_h;
  // tiles of whole genes, each with at most max_chunks chunks (one gene at least), as in pb_sparse
  int64_t need = 1;
  for (int64_t g0 = 0; g0 < G;) {
    int64_t g1 = g0 + 1;
    while (g1 < G && gc[(size_t)g1 + 1] - gc[(size_t)g0] <= max_chunks) ++g1;
    need = std::max(need, gc[(size_t)g1] - gc[(size_t)g0]);
    g0 = g1;
  }
  if (need > 0x7fffffffll) CNA_FAIL(CNA_EINVAL, "cna_expr_cross: one gene has too many chunks");
  CNA_TRY(buf_need(c, s, s->xpart, 8 * need * Nx));
  CNA_TRY(buf_need(c, s, s->xpart2, 16 * std::max<int64_t>(1, s->nchunks)));
  for (int64_t g0 = 0; g0 < G;) {
    int64_t g1 = g0 + 1;
    while (g1 < G && gc[(size_t)g1 + 1] - gc[(size_t)g0] <= max_chunks) ++g1;
    const int64_t c0 = gc[(size_t)g0], nch = gc[(size_t)g1] - c0;
    if (nch) {
      if (Nx <= 64) xc_sparse_launch<T, 1>(s, nch, c0, Xw, ldx, Nx);
      else if (Nx <= 128) xc_sparse_launch<T, 2>(s, nch, c0, Xw, ldx, Nx);
      else if (Nx <= 256) xc_sparse_launch<T, 4>(s, nch, c0, Xw, ldx, Nx);
      else if (Nx <= 512) xc_sparse_launch<T, 8>(s, nch, c0, Xw, ldx, Nx);
      else xc_sparse_launch<T, 16>(s, nch, c0, Xw, ldx, Nx);
    }
    hipLaunchKernelGGL(k_xc_finish_sparse, dim3((unsigned)(((g1 - g0) * Nx + 255) / 256)), dim3(256), 0, s->st,
                       (const double*)s->xpart.p, (const int64_t*)s->gchunk.p, g0, g1, c0, Nx, W);
    g0 = g1;
  }
  hipLaunchKernelGGL(k_xc_finish_sparse_sx, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s->st, (const double*)s->xpart2.p,
                     (const int64_t*)s->gchunk.p, G, sx, sx + G);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

int devbuf_free(cna_ctx* c, DevBuf& b) {
  if (b.p) dev_free(c, b.p, (size_t)b.cap);
  b.p = nullptr;
  b.cap = 0;
  return 0;
}

int devbuf_need(cna_ctx* c, hipStream_t st, DevBuf& b, int64_t bytes) {
  if (b.p && b.cap >= bytes) return 0;
  if (b.p) {
    HIP_TRY(hipStreamSynchronize(st));
    devbuf_free(c, b);
  }
  if (bytes < 256) bytes = 256;
  CNA_TRY(dev_alloc(c, &b.p, (size_t)bytes));
  b.cap = bytes;
  return 0;
}

void launch_block_scan(hipStream_t st, unsigned int* cnt, int64_t G, int B, int64_t* total) {
  hipLaunchKernelGGL(k_tr_scan, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, cnt, G, B, total);
}

int expr_stream(cna_ctx* c, hipStream_t* st) {
  ExprState* s = nullptr;
  CNA_TRY(get_state(c, &s));
  *st = s->st;
  return 0;
}

void expr_destroy(cna_ctx* c) {
  ExprState* s = state_of(c);
  if (!s) return;
  release_matrix(c, s);
  strata_release(c, s->st);
  if (s->st) (void)hipStreamDestroy(s->st);
  if (s->x_ready) (void)hipEventDestroy(s->x_ready);
  delete s;
  c->expr = nullptr;
}

extern "C" {

int cna_expr_drop(cna_ctx* c) {
  CHECK_CTX(c);
  if (state_of(c)) {
    release_matrix(c, state_of(c));
    strata_release(c, state_of(c)->st);
  }
  return 0;
}

int cna_expr_shape(cna_ctx* c, int64_t* n_cells, int64_t* n_genes, int64_t* nnz, int* format, int* is_f64, int64_t* n_uploads) {
  CHECK_CTX(c);
  const ExprState* s = state_of(c);
  if (n_cells) *n_cells = s ? s->n : 0;
  if (n_genes) *n_genes = s ? s->G : 0;
  if (nnz) *nnz = s ? s->nnz : 0;
  if (format) *format = s ? s->format : 0;
  if (is_f64) *is_f64 = s ? s->is_f64 : 0;
  if (n_uploads) *n_uploads = s ? s->n_uploads : 0;
  return 0;
}

int cna_expr_upload_dense(cna_ctx* c, const void* x, int64_t n_cells, int64_t n_genes, int is_f64) {
  CHECK_CTX(c);
  if (!x) CNA_FAIL(CNA_EINVAL, "expression matrix: null pointer");
  if (n_cells < 1 || n_genes < 1 || n_cells >= (1ll << 31) || n_genes >= (1ll << 31))
    CNA_FAIL(CNA_EINVAL, "expression matrix: cells and genes must lie in [1, 2^31)");
  ExprState* s = nullptr;
  CNA_TRY(get_state(c, &s));
  release_matrix(c, s);
  const int64_t bytes = n_cells * n_genes * (is_f64 ? 8 : 4);
  int rc = buf_need(c, s, s->X, bytes);
  if (rc != 0) {
    release_matrix(c, s);
    if (rc == CNA_ENOMEM)
      cna_set_error("expression matrix: " + std::to_string(bytes) + " bytes do not fit on the device; nothing is resident");
    return rc;
  }
  hipError_t e = hipMemcpyAsync(s->X.p, x, (size_t)bytes, hipMemcpyHostToDevice, s->st);
  if (e == hipSuccess) e = hipStreamSynchronize(s->st);
  if (e != hipSuccess) {
    release_matrix(c, s);
    cna_set_error(std::string("expression matrix upload: ") + hipGetErrorString(e));
    return (int)e;
  }
  s->format = 1;
  s->is_f64 = is_f64 != 0;
  s->n = n_cells; s->G = n_genes; s->nnz = n_cells * n_genes;
  s->n_uploads += 1;
  return 0;
}

int cna_expr_upload_sparse(cna_ctx* c, const void* indptr, const void* indices, const void* data, int64_t n_cells,
                           int64_t n_genes, int64_t nnz, int index_bytes, int is_f64, int is_csc) {
  CHECK_CTX(c);
  if (!indptr || (nnz > 0 && (!indices || !data))) CNA_FAIL(CNA_EINVAL, "expression matrix: null pointer");
  if (n_cells < 1 || n_genes < 1 || n_cells >= (1ll << 31) || n_genes >= (1ll << 31) || nnz < 0)
    CNA_FAIL(CNA_EINVAL, "expression matrix: cells and genes must lie in [1, 2^31), nnz in [0, 2^63)");
  if (index_bytes != 4 && index_bytes != 8) CNA_FAIL(CNA_EINVAL, "expression matrix: indices take 4 or 8 bytes");
  ExprState* s = nullptr;
  CNA_TRY(get_state(c, &s));
  release_matrix(c, s);
  const int rc = upload_sparse(c, s, indptr, indices, data, n_cells, n_genes, nnz, index_bytes, is_f64 != 0, is_csc != 0);
  if (rc != 0) {
    const std::string why = cna_last_error();
    release_matrix(c, s);
    if (rc == CNA_ENOMEM)
      cna_set_error("expression matrix: the device has no room for the gene-major copy" +
                    std::string(is_csc ? "" : " and the rows it is transposed from") + " (" + why + "); nothing is resident");
    return rc;
  }
  s->format = 2;
  s->n_uploads += 1;
  return 0;
}

int cna_gene_corr(cna_ctx* c, const double* V, int q, double* r_out) {
  CHECK_CTX(c);
  ExprState* s = state_of(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, "cna_gene_corr: no expression matrix is resident (cna_expr_upload_*)");
  if (!V || !r_out) CNA_FAIL(CNA_EINVAL, "cna_gene_corr: null pointer");
  if (q < 1 || q > GC_MAXQ) CNA_FAIL(CNA_EINVAL, "cna_gene_corr: 1 <= q <= 16 key columns");
  int Q = 1;
  while (Q < q) Q *= 2;
  const int64_t n = s->n, G = s->G;
  CNA_TRY(buf_need(c, s, s->vraw, 8 * n * q));
  CNA_TRY(buf_need(c, s, s->vtab, 8 * n * Q));
  CNA_TRY(buf_need(c, s, s->vmask, 4 * n));
  CNA_TRY(buf_need(c, s, s->kstat, 8 * KS_LD * GC_MAXQ));
  CNA_TRY(buf_need(c, s, s->flag, 256));
  CNA_TRY(buf_need(c, s, s->rout, 8 * G * q));
  HIP_TRY(hipMemcpyAsync(s->vraw.p, V, (size_t)(8 * n * q), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipMemsetAsync(s->flag.p, 0, 4, s->st));
  hipLaunchKernelGGL(k_key_stats, dim3(q), dim3(1024), 0, s->st, (const double*)s->vraw.p, n, (double*)s->kstat.p);
  hipLaunchKernelGGL(k_key_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->st, (const double*)s->vraw.p, n, q, Q,
                     (const double*)s->kstat.p, (double*)s->vtab.p, (uint32_t*)s->vmask.p, (int*)s->flag.p);
  HIP_TRY(hipGetLastError());
  // keys that leave out the same cells (usually none) share the sums of x and x^2: one set instead of q
  int differ = 0;
  HIP_TRY(hipMemcpyAsync(&differ, s->flag.p, 4, hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  const bool shared = differ == 0;
  const int S = shared ? 1 : Q;
  if (s->format == 1) {
    const int F = 4 * S + Q;
    // slabs: enough single-wave workgroups to fill the device, partial records at most ~2 % of the matrix' bytes
    const int64_t gene_blocks = (G + 63) / 64;
    int64_t nslab = std::min<int64_t>(2048, (8192 + gene_blocks - 1) / gene_blocks);
    nslab = std::max<int64_t>(1, std::min<int64_t>(nslab, n / (100 * (int64_t)F)));
    const int64_t slab_rows = (n + nslab - 1) / nslab;
    nslab = (n + slab_rows - 1) / slab_rows;
    CNA_TRY(buf_need(c, s, s->part, 8 * nslab * F * G));
    if (s->is_f64) launch_pass<double>(s, Q, shared, (int)nslab, slab_rows);
    else launch_pass<float>(s, Q, shared, (int)nslab, slab_rows);
    hipLaunchKernelGGL(k_gc_finish_dense, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s->st, (const double*)s->part.p, G,
                       (int)nslab, q, Q, S, (const double*)s->kstat.p, (double*)s->rout.p);
  } else {
    const int F = 5 * S + Q;
    CNA_TRY(buf_need(c, s, s->part, 8 * std::max<int64_t>(1, s->nchunks) * F));
    if (s->nchunks) {
      if (s->is_f64) launch_pass<double>(s, Q, shared, 0, 0);
      else launch_pass<float>(s, Q, shared, 0, 0);
    }
    hipLaunchKernelGGL(k_gc_finish_sparse, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s->st, (const double*)s->part.p,
                       (const int64_t*)s->gchunk.p, G, q, Q, S, (const double*)s->kstat.p, (double*)s->rout.p);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(r_out, s->rout.p, (size_t)(8 * G * q), hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  return 0;
}

int cna_expr_to_bins(cna_ctx* c, const int32_t* codes, int n_bins, int what, double* sums_out, int64_t* counts_out) {
  CHECK_CTX(c);
  ExprState* s = state_of(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, "cna_expr_to_bins: no expression matrix is resident (cna_expr_upload_*)");
  if (!codes || !sums_out || !counts_out) CNA_FAIL(CNA_EINVAL, "cna_expr_to_bins: null pointer");
  if (n_bins < 1 || n_bins > PB_MAX_BINS) CNA_FAIL(CNA_EINVAL, "cna_expr_to_bins: 1 <= n_bins <= 4096");
  if (what != 0 && what != 1) CNA_FAIL(CNA_EINVAL, "cna_expr_to_bins: what is 0 (sums of x) or 1 (counts of x > 0)");
  const int64_t n = s->n, G = s->G;
  const int64_t rpb = round_up64((n + PB_MAX_BLOCKS - 1) / PB_MAX_BLOCKS, 64);
  const int64_t B = (n + rpb - 1) / rpb;
  CNA_TRY(buf_need(c, s, s->bcode, 4 * n));
  CNA_TRY(buf_need(c, s, s->bcnt, 4 * B * n_bins));
  CNA_TRY(buf_need(c, s, s->btot, 8 * (int64_t)n_bins));
  CNA_TRY(buf_need(c, s, s->flag, 256));
  CNA_TRY(buf_need(c, s, s->rout, 8 * G * n_bins));
  HIP_TRY(hipMemcpyAsync(s->bcode.p, codes, (size_t)(4 * n), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipMemsetAsync(s->flag.p, 0, 4, s->st));
  hipLaunchKernelGGL(k_pb_count, dim3((unsigned)B), dim3(256), 0, s->st, (const int32_t*)s->bcode.p, n, n_bins, rpb,
                     (unsigned int*)s->bcnt.p, (int*)s->flag.p);
  hipLaunchKernelGGL(k_tr_scan, dim3((unsigned)((n_bins + 255) / 256)), dim3(256), 0, s->st, (unsigned int*)s->bcnt.p,
                     (int64_t)n_bins, (int)B, (int64_t*)s->btot.p);
  HIP_TRY(hipGetLastError());
  // the codes are judged before any sum is formed
  int bad = 0;
  std::vector<int64_t> tot((size_t)n_bins);
  HIP_TRY(hipMemcpyAsync(&bad, s->flag.p, 4, hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipMemcpyAsync(tot.data(), s->btot.p, 8 * (size_t)n_bins, hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  if (bad) CNA_FAIL(CNA_EINVAL, "cna_expr_to_bins: a code lies outside [-1, n_bins)");
  if (s->format == 1)
    CNA_TRY(s->is_f64 ? pb_dense<double>(c, s, n_bins, what == 1, tot) : pb_dense<float>(c, s, n_bins, what == 1, tot));
  else
    CNA_TRY(s->is_f64 ? pb_sparse<double>(c, s, n_bins, what == 1) : pb_sparse<float>(c, s, n_bins, what == 1));
  HIP_TRY(hipMemcpyAsync(sums_out, s->rout.p, (size_t)(8 * G * n_bins), hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  std::memcpy(counts_out, tot.data(), 8 * (size_t)n_bins);
  return 0;
}

int cna_expr_cross(cna_ctx* c, const int64_t* xrow, int64_t n_cells, double* W_out, double* rho_out, double* sx_out,
                   double* sxx_out, int64_t* m_out) {
  CHECK_CTX(c);
  ExprState* s = state_of(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, "cna_expr_cross: no expression matrix is resident (cna_expr_upload_*)");
  if (c->auto_pending) CNA_TRY(cna_nam_auto_finish(c, nullptr, nullptr));
  if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "cna_expr_cross: X not available");
  if (comm_active(c)) CNA_FAIL(CNA_ESTATE, "cna_expr_cross: one rank only (the rows of X of other ranks are not here)");
  if (!xrow || !W_out || !rho_out || !sx_out || !sxx_out || !m_out) CNA_FAIL(CNA_EINVAL, "cna_expr_cross: null pointer");
  if (n_cells != s->n)
    CNA_FAIL(CNA_EINVAL, "cna_expr_cross: xrow has " + std::to_string(n_cells) + " entries, the expression matrix " +
                             std::to_string(s->n) + " cells");
  const int64_t n = s->n, G = s->G, nx = c->nx;
  const int Nx = c->Nx, ldx = c->ldx;
  if (Nx < 1 || Nx > XC_MAX_COLS) CNA_FAIL(CNA_EINVAL, "cna_expr_cross: 1 <= columns of X <= 1024");
  const double* Xw = c->X;
  const int64_t n_out = G * Nx + Nx + 2 * G;
  CNA_TRY(buf_need(c, s, s->xrow, 8 * n));
  CNA_TRY(buf_need(c, s, s->xseen, 4 * std::max<int64_t>(1, nx)));
  CNA_TRY(buf_need(c, s, s->flag, 256));
  CNA_TRY(buf_need(c, s, s->xout, 8 * n_out));
  HIP_TRY(hipMemcpyAsync(s->xrow.p, xrow, (size_t)(8 * n), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipMemsetAsync(s->xseen.p, 0, (size_t)(4 * std::max<int64_t>(1, nx)), s->st));
  HIP_TRY(hipMemsetAsync(s->flag.p, 0, 16, s->st));
  hipLaunchKernelGGL(k_xc_check, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, s->st,
                     (const int64_t*)s->xrow.p, n, nx, (unsigned int*)s->xseen.p, (int*)s->flag.p,
                     (unsigned long long*)((char*)s->flag.p + 8));
  HIP_TRY(hipGetLastError());
  // xrow is judged before any sum is formed (and before X is touched)
  int64_t verdict[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(verdict, s->flag.p, 16, hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  const int bad = (int)(verdict[0] & 0xffffffffll);
  if (bad & 1) CNA_FAIL(CNA_EINVAL, "cna_expr_cross: an xrow lies outside [-1, rows of X)");
  if (bad & 2) CNA_FAIL(CNA_EINVAL, "cna_expr_cross: two cells name the same row of X");
  // whatever the main stream has queued that produces X comes first (an event, no host sync).  The other direction needs
  // nothing: this entry returns only after the expression stream has drained, so a later producer of X finds the read done
  HIP_TRY(hipEventRecord(s->x_ready, c->stream));
  HIP_TRY(hipStreamWaitEvent(s->st, s->x_ready, 0));
  double* W = (double*)s->xout.p;
  double* rho = W + G * Nx;
  double* sx = rho + Nx;
  int rc;
  if (s->format == 1) rc = s->is_f64 ? xc_dense<double>(c, s, Xw, ldx, Nx, W, sx) : xc_dense<float>(c, s, Xw, ldx, Nx, W, sx);
  else rc = s->is_f64 ? xc_sparse<double>(c, s, Xw, ldx, Nx, W, sx) : xc_sparse<float>(c, s, Xw, ldx, Nx, W, sx);
  if (rc == 0) {
    const int64_t rpb = std::max<int64_t>(256, (n + 1023) / 1024);
    const int64_t B = (n + rpb - 1) / rpb;
    rc = buf_need(c, s, s->xrpart, 8 * B * Nx);
    if (rc == 0) {
      hipLaunchKernelGGL(k_xc_rho, dim3((unsigned)B), dim3(256), 0, s->st, (const int64_t*)s->xrow.p, n, rpb, Xw, ldx, Nx,
                         (double*)s->xrpart.p);
      hipLaunchKernelGGL(k_xc_fold, dim3((unsigned)((Nx + 255) / 256)), dim3(256), 0, s->st, (const double*)s->xrpart.p,
                         (int64_t)Nx, (int)B, rho);
    }
  }
  if (rc != 0) {
    (void)hipStreamSynchronize(s->st);
    return rc;
  }
  std::vector<double> host((size_t)n_out);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(host.data(), s->xout.p, (size_t)(8 * n_out), hipMemcpyDeviceToHost, s->st);
  const hipError_t e2 = hipStreamSynchronize(s->st);
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) {
    cna_set_error(std::string("cna_expr_cross: ") + hipGetErrorString(e));
    return (int)e;
  }
  std::memcpy(W_out, host.data(), 8 * (size_t)(G * Nx));
  std::memcpy(rho_out, host.data() + G * Nx, 8 * (size_t)Nx);
  std::memcpy(sx_out, host.data() + G * Nx + Nx, 8 * (size_t)G);
  std::memcpy(sxx_out, host.data() + G * Nx + Nx + G, 8 * (size_t)G);
  *m_out = verdict[1];
  return 0;
}

}  // extern "C"

// cna_gene_corr: per-gene Pearson correlation to per-cell columns (the neighbourhood coefficient of cna.tl.association,
// NAM PC loadings, ...) over the resident expression matrix (genes.hip).  Replaces the host line of the reference's
// workflow (demo/demo.ipynb, "per-gene correlations to neighborhood coefficient"):
//     d.var['corr_case'] = np.corrcoef(d.obs.male_coef.values.reshape(1,-1), d.X, rowvar=False)[0,1:]
// The key columns are in the CALLER's cell order, as the matrix is.
//
//   k_key_stats     (expr.h) per key column: finite count, mean, sum (v - mean), sum (v - mean)^2, min, max (fixed-order sums)
//   k_key_table     cells x Q table of centred key values (0 where the cell is left out) + one mask word per cell
//   k_gc_dense      X is cells x genes: lane = gene, a wave walks down a slab of cells (coalesced rows, the key values
//                   of a cell are wave-uniform); partial sums per slab with plain stores
//   k_gc_sparse     gene-major lists {cell, value}: one wave per chunk of a gene's list, gathers the cell's table row;
//                   partial sums per chunk with plain stores
//   k_gc_finish_*   adds the partials of a gene in slab / chunk order and turns them into r
//
// Result sums take a fixed order (no floating-point atomics): two runs on one input give the same bits.
#include "expr.h"
#include <cmath>

namespace {

constexpr int GC_MAXQ = 16;

// raw key columns, their table and masks, the key statistics, the partial records, r, the "masks differ" word
struct CorrWork : BufSet {
  Buf vraw{*this}, vtab{*this}, vmask{*this}, kstat{*this}, part{*this}, rout{*this}, flag{*this};
};

// ------------------------------------------------------------------ key columns (k_key_stats: expr.h)
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
    const double a = wave_sum(sx[s]), b = wave_sum(sxx[s]), c0 = wave_min(mn[s]), c1 = wave_max(mx[s]),
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

// one pass over the matrix: the kernel for its form, its element type, Q and whether the keys share one mask
void launch_pass(ExprState* s, CorrWork* w, int Q, bool shared, int nslab, int64_t slab_rows) {
  with_bool(s->is_f64 != 0, [&](auto f64) {
    using T = std::conditional_t<decltype(f64)::value, double, float>;
    with_width(Q, [&](auto width) {
      with_bool(shared, [&](auto sh) {
        constexpr int QQ = decltype(width)::value;
        constexpr bool SH = decltype(sh)::value;
        if (s->format == 1)
          hipLaunchKernelGGL((k_gc_dense<T, QQ, SH>), dim3((unsigned)((s->G + 63) / 64), (unsigned)nslab), dim3(64), 0, s->st,
                             s->X.as<const T>(), s->n, s->G, slab_rows, w->vtab.as<const double>(),
                             w->vmask.as<const uint32_t>(), w->part.as<double>());
        else
          hipLaunchKernelGGL((k_gc_sparse<T, QQ, SH>), dim3((unsigned)((s->nchunks + 3) / 4)), dim3(256), 0, s->st,
                             s->chunk_lo.as<const int64_t>(), s->chunk_gene.as<const int32_t>(), s->gptr.as<const int64_t>(),
                             s->nchunks, s->chunk_len, s->gcell.as<const int32_t>(), s->gval.as<const T>(),
                             w->vtab.as<const double>(), w->vmask.as<const uint32_t>(), w->part.as<double>());
      });
    });
  });
}

}  // namespace

extern "C" int cna_gene_corr(cna_ctx* c, const double* V, int q, double* r_out) {
  CHECK_CTX(c);
  ExprState* s = expr_state(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, "cna_gene_corr: no expression matrix is resident (cna_expr_upload_*)");
  if (!V || !r_out) CNA_FAIL(CNA_EINVAL, "cna_gene_corr: null pointer");
  if (q < 1 || q > GC_MAXQ) CNA_FAIL(CNA_EINVAL, "cna_gene_corr: 1 <= q <= 16 key columns");
  int Q = 1;
  while (Q < q) Q *= 2;
  const int64_t n = s->n, G = s->G;
  CorrWork* w = expr_work<CorrWork>(s, EXPR_CORR);
  CNA_TRY(buf_need(c, s->st, w->vraw, 8 * n * q));
  CNA_TRY(buf_need(c, s->st, w->vtab, 8 * n * Q));
  CNA_TRY(buf_need(c, s->st, w->vmask, 4 * n));
  CNA_TRY(buf_need(c, s->st, w->kstat, 8 * KS_LD * GC_MAXQ));
  CNA_TRY(buf_need(c, s->st, w->flag, 256));
  CNA_TRY(buf_need(c, s->st, w->rout, 8 * G * q));
  HIP_TRY(hipMemcpyAsync(w->vraw.p, V, (size_t)(8 * n * q), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipMemsetAsync(w->flag.p, 0, 4, s->st));
  hipLaunchKernelGGL(k_key_stats, dim3(q), dim3(1024), 0, s->st, (const double*)w->vraw.p, n, (double*)w->kstat.p);
  hipLaunchKernelGGL(k_key_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->st, (const double*)w->vraw.p, n, q, Q,
                     (const double*)w->kstat.p, (double*)w->vtab.p, (uint32_t*)w->vmask.p, (int*)w->flag.p);
  HIP_TRY(hipGetLastError());
  // keys that leave out the same cells (usually none) share the sums of x and x^2: one set instead of q
  int differ = 0;
  HIP_TRY(hipMemcpyAsync(&differ, w->flag.p, 4, hipMemcpyDeviceToHost, s->st));
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
    CNA_TRY(buf_need(c, s->st, w->part, 8 * nslab * F * G));
    launch_pass(s, w, Q, shared, (int)nslab, slab_rows);
    hipLaunchKernelGGL(k_gc_finish_dense, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s->st, (const double*)w->part.p, G,
                       (int)nslab, q, Q, S, (const double*)w->kstat.p, (double*)w->rout.p);
  } else {
    const int F = 5 * S + Q;
    CNA_TRY(buf_need(c, s->st, w->part, 8 * std::max<int64_t>(1, s->nchunks) * F));
    if (s->nchunks) launch_pass(s, w, Q, shared, 0, 0);
    hipLaunchKernelGGL(k_gc_finish_sparse, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s->st, (const double*)w->part.p,
                       (const int64_t*)s->gchunk.p, G, q, Q, S, (const double*)w->kstat.p, (double*)w->rout.p);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(r_out, w->rout.p, (size_t)(8 * G * q), hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  return 0;
}

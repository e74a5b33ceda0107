// cna_expr_cross: the resident expression matrix against the working matrix X (cna.tl.gene_test): W = E_K^T X, genes x
// samples, the one cell-sized contraction behind the null correlations of every gene with the permuted phenotypes'
// coefficients c_p = X^T z_p / N (the reference's null of _association.py:94-99; the observed coefficient is its line 77,
// and the per-gene correlation demo/demo.ipynb's "per-gene correlations to neighborhood coefficient").  The only entry
// of the expression side that reads the state of c_api.hip (X, read-only).
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
// Result sums take a fixed order (no floating-point atomics): two runs on one input give the same bits.
#include "expr.h"
#include <cstring>

namespace {

// xrow, the table of named X rows, the verdict, partial sums (W | sum x, sum x^2 | column sums), the results
struct CrossWork : BufSet {
  Buf xrow{*this}, xseen{*this}, flag{*this}, xpart{*this}, xpart2{*this}, xrpart{*this}, xout{*this};
};

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
int xc_dense(cna_ctx* c, ExprState* s, CrossWork* w, const double* Xw, int ldx, int Nx, double* W, double* sx) {
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
  CNA_TRY(buf_need(c, s->st, w->xpart, 8 * nslab * Nx * G));
  CNA_TRY(buf_need(c, s->st, w->xpart2, 16 * nslab * G));
  hipLaunchKernelGGL((k_xc_dense<T>), dim3((unsigned)(gene_blocks * ntile), (unsigned)nslab), dim3(64), 0, s->st,
                     (const T*)s->X.p, n, G, slab_rows, (const int64_t*)w->xrow.p, Xw, ldx, Nx, ntile, (double*)w->xpart.p,
                     (double*)w->xpart2.p);
  hipLaunchKernelGGL(k_xc_finish_dense, dim3((unsigned)((G * Nx + 255) / 256)), dim3(256), 0, s->st, (const double*)w->xpart.p,
                     G, Nx, (int)nslab, W);
  hipLaunchKernelGGL(k_xc_fold, dim3((unsigned)((2 * G + 255) / 256)), dim3(256), 0, s->st, (const double*)w->xpart2.p, 2 * G,
                     (int)nslab, sx);
  HIP_TRY(hipGetLastError());
  return 0;
}

template <typename T>
int xc_sparse(cna_ctx* c, ExprState* s, CrossWork* w, const double* Xw, int ldx, int Nx, double* W, double* sx) {
  int64_t need = 1;
  const std::vector<GeneTile> tiles = gene_tiles(s, 8 * (int64_t)Nx, &need);
  if (need > 0x7fffffffll) CNA_FAIL(CNA_EINVAL, "cna_expr_cross: one gene has too many chunks");
  CNA_TRY(buf_need(c, s->st, w->xpart, 8 * need * Nx));
  CNA_TRY(buf_need(c, s->st, w->xpart2, 16 * std::max<int64_t>(1, s->nchunks)));
  for (const GeneTile& t : tiles) {
    if (t.nch)
      with_width((Nx + 63) / 64, [&](auto width) {
        hipLaunchKernelGGL((k_xc_sparse<T, decltype(width)::value>), dim3((unsigned)t.nch), dim3(64), 0, s->st,
                           s->chunk_lo.as<const int64_t>(), s->chunk_gene.as<const int32_t>(), s->gptr.as<const int64_t>(), t.c0,
                           s->chunk_len, s->gcell.as<const int32_t>(), s->gval.as<const T>(), w->xrow.as<const int64_t>(), Xw, ldx,
                           Nx, w->xpart.as<double>(), w->xpart2.as<double>());
      });
    hipLaunchKernelGGL(k_xc_finish_sparse, dim3((unsigned)(((t.g1 - t.g0) * Nx + 255) / 256)), dim3(256), 0, s->st,
                       w->xpart.as<const double>(), s->gchunk.as<const int64_t>(), t.g0, t.g1, t.c0, Nx, W);
  }
  hipLaunchKernelGGL(k_xc_finish_sparse_sx, dim3((unsigned)((s->G + 255) / 256)), dim3(256), 0, s->st,
                     w->xpart2.as<const double>(), s->gchunk.as<const int64_t>(), s->G, sx, sx + s->G);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

// expr.h: the verdict on a map cells -> rows of X, for every entry that takes one
int xrow_check(cna_ctx* c, hipStream_t st, const int64_t* xrow_dev, int64_t n, int64_t nx, Buf& seen, Buf& flag,
               const char* who, int64_t* m) {
  CNA_TRY(buf_need(c, st, seen, 4 * std::max<int64_t>(1, nx)));
  CNA_TRY(buf_need(c, st, flag, 256));
  HIP_TRY(hipMemsetAsync(seen.p, 0, (size_t)(4 * std::max<int64_t>(1, nx)), st));
  HIP_TRY(hipMemsetAsync(flag.p, 0, 16, st));
  hipLaunchKernelGGL(k_xc_check, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, xrow_dev, n, nx,
                     seen.as<unsigned int>(), flag.as<int>(), (unsigned long long*)((char*)flag.p + 8));
  HIP_TRY(hipGetLastError());
  int64_t verdict[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(verdict, flag.p, 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int bad = (int)(verdict[0] & 0xffffffffll);
  if (bad & 1) CNA_FAIL(CNA_EINVAL, std::string(who) + ": an xrow lies outside [-1, rows of X)");
  if (bad & 2) CNA_FAIL(CNA_EINVAL, std::string(who) + ": two cells name the same row of X");
  *m = verdict[1];
  return 0;
}

extern "C" int cna_expr_cross(cna_ctx* c, const int64_t* xrow, int64_t n_cells, double* W_out, double* rho_out, double* sx_out,
                   double* sxx_out, int64_t* m_out) {
  CHECK_CTX(c);
  ExprState* s = expr_state(c);
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
  CrossWork* w = expr_work<CrossWork>(s, EXPR_CROSS);
  const int64_t n_out = G * Nx + Nx + 2 * G;
  CNA_TRY(buf_need(c, s->st, w->xrow, 8 * n));
  CNA_TRY(buf_need(c, s->st, w->xout, 8 * n_out));
  HIP_TRY(hipMemcpyAsync(w->xrow.p, xrow, (size_t)(8 * n), hipMemcpyHostToDevice, s->st));
  // xrow is judged before any sum is formed (and before X is touched)
  int64_t m = 0;
  CNA_TRY(xrow_check(c, s->st, w->xrow.as<const int64_t>(), n, nx, w->xseen, w->flag, "cna_expr_cross", &m));
  // whatever the main stream has queued that produces X comes first (an event, no host sync).  The other direction needs
  // nothing: this entry returns only after the expression stream has drained, so a later producer of X finds the read done
  HIP_TRY(hipEventRecord(s->x_ready, c->stream));
  HIP_TRY(hipStreamWaitEvent(s->st, s->x_ready, 0));
  double* W = (double*)w->xout.p;
  double* rho = W + G * Nx;
  double* sx = rho + Nx;
  int rc;
  if (s->format == 1) rc = s->is_f64 ? xc_dense<double>(c, s, w, Xw, ldx, Nx, W, sx) : xc_dense<float>(c, s, w, Xw, ldx, Nx, W, sx);
  else rc = s->is_f64 ? xc_sparse<double>(c, s, w, Xw, ldx, Nx, W, sx) : xc_sparse<float>(c, s, w, Xw, ldx, Nx, W, sx);
  if (rc == 0) {
    const int64_t rpb = std::max<int64_t>(256, (n + 1023) / 1024);
    const int64_t B = (n + rpb - 1) / rpb;
    rc = buf_need(c, s->st, w->xrpart, 8 * B * Nx);
    if (rc == 0) {
      hipLaunchKernelGGL(k_xc_rho, dim3((unsigned)B), dim3(256), 0, s->st, (const int64_t*)w->xrow.p, n, rpb, Xw, ldx, Nx,
                         (double*)w->xrpart.p);
      hipLaunchKernelGGL(k_xc_fold, dim3((unsigned)((Nx + 255) / 256)), dim3(256), 0, s->st, (const double*)w->xrpart.p,
                         (int64_t)Nx, (int)B, rho);
    }
  }
  if (rc != 0) {
    (void)hipStreamSynchronize(s->st);
    return rc;
  }
  std::vector<double> host((size_t)n_out);
  CNA_TRY(fetch_results(s->st, "cna_expr_cross", {{host.data(), w->xout.p, (size_t)(8 * n_out)}}));
  std::memcpy(W_out, host.data(), 8 * (size_t)(G * Nx));
  std::memcpy(rho_out, host.data() + G * Nx, 8 * (size_t)Nx);
  std::memcpy(sx_out, host.data() + G * Nx + Nx, 8 * (size_t)G);
  std::memcpy(sxx_out, host.data() + G * Nx + Nx + G, 8 * (size_t)G);
  *m_out = m;
  return 0;
}

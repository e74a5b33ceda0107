// cna_nbhd_expr, cna_gene_nbhd_corr: the expression of a NEIGHBOURHOOD -- the mean of a gene over the cells that the
// nsteps-step random walk anchored at a cell reaches, with the weights the NAM uses -- and its Pearson correlation to
// per-cell columns (the neighbourhood coefficient).  With one walk step (reference _nam.py:28-33)
//     c = A.sum(0) + w,     P s = A.(s/c) + w*s/c
// and e_g the column of gene g of the resident expression matrix widened to float64,
//     m_g = (P^nsteps e_g) / (P^nsteps 1)            element-wise
// The numerator is what the NAM would hold if the gene were a sample, the denominator the membership mass of the
// neighbourhood.  A cell whose denominator is not a positive finite number is left out of every sum; its m is NaN.
//
// The numerator columns and the denominator are, bit for bit, what the dense walk (cna_dense_load / cna_dense_step,
// diffuse.hip: k_scale_rows, k_nam_step, k_nam_step_pair) makes of the same columns: the quotient s/c first (a
// correctly rounded division), then per row the stored entries in stored order, a multiply and then an add -- this
// file does not contract either -- then + w * the row's own entry, then the division for the next step.  Columns of a
// walk do not mix, so the width of a tile changes nothing.
//
// Nothing here writes the state of c_api.hip: the graph, the device cell order and the column sums are read where they
// are (as components.hip reads them), the buffers are this file's own (NbhdWork, slot EXPR_NBHD, freed by
// cna_expr_drop), the stream is the expression stream, which waits for what the main stream has queued.
//
// Genes go in tiles of TW columns (64, or 32 with two rows per wave); a tile is n x TW float64 in the DEVICE's row order:
//   k_nx_inverse      inv[orig_idx[i]] = i, once per call (gene-major lists only)
//   k_nx_fill_dense   t[i][c] = X[orig_idx[i]][gene c] / c[i]
//   k_nx_fill_lists   a cleared tile, then the entries of the tile's genes scattered through inv
//   k_nx_fill_ones    the ones column (c = 0 of a tile)
//   k_nx_step         lane = column: the row's entries in stored order, U neighbour rows in flight; writes the scaled
//                     state, or the unscaled one after the last step; two tiles, ping-pong
//   k_nx_unpermute    columns of a tile -> an array in the caller's order (or, without an order, a plain copy)
//   k_nx_keys         the key columns in the device's order, NaN where the denominator is bad; k_key_stats (expr.h) on them
//   k_nx_keytab       cells x Q centred key values and one mask word per cell
//   k_nx_pass1        m = s / den in place; per slab of rows, column and key the sum of m          (partials, plain stores)
//   k_nx_mean         adds them in a fixed order (one wave per (key, column)) -> the mean of m
//   k_nx_pass2        per slab: sum (m - mean)^2, sum (m - mean)(v - mean v)
//   k_nx_finish       adds them in the same fixed order -> r, mean, sd
//   k_nx_range_*      minimum and maximum of every gene over ALL cells of the raw matrix (implicit zeros counted): a
//                     constant gene is decided exactly, not from m (smoothing 3.0 does not give back 3.0 exactly)
// No floating-point atomics: two runs give the same bits.
#include "expr.h"
#include <chrono>
#include <cmath>
#include <cstdlib>

// the walk's rounding sequence: a multiply, then an add (diffuse.hip does the same)
#pragma clang fp contract(off)

namespace {

constexpr int NB_MAXQ = 16;
constexpr int NB_MAX_GENES = 64;     // cna_nbhd_expr: one tile
constexpr int NB_MAX_STEPS = 15;
constexpr int NB_U = 8;              // neighbour rows in flight per lane
constexpr int64_t NB_SLABS = 4096;   // slabs of rows of the moments passes (at least NB_MIN_SLAB rows each)
constexpr int64_t NB_MIN_SLAB = 16;
constexpr int NB_RANGE_SLABS = 256;

struct NbhdWork : BufSet {
  Buf ta{*this}, tb{*this};            // the two tiles, n x TW float64
  Buf den{*this};                      // P^nsteps 1, device order
  Buf inv{*this};                      // device row of every caller's cell
  Buf glist{*this};                    // cna_nbhd_expr: the chosen genes
  Buf out{*this};                      // cna_nbhd_expr: numerators and denominator in the caller's order
  Buf vraw{*this}, vdev{*this}, vtab{*this}, vmask{*this}, kstat{*this};
  Buf part{*this}, mean{*this}, range{*this}, flag{*this}, res{*this};
};

__device__ __forceinline__ bool nb_good(double den) { return den > 0.0 && finite_d(den); }

__global__ __launch_bounds__(256) void k_nx_inverse(const int64_t* __restrict__ orig, int64_t n, int32_t* __restrict__ inv) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t o = orig ? orig[i] : i;
  if (o >= 0 && o < n) inv[o] = (int32_t)i;
}

// gene of column c of a tile: a list (cna_nbhd_expr) or g0 + c
__device__ __forceinline__ int64_t nb_gene(const int32_t* __restrict__ glist, int64_t g0, int c) {
  return glist ? (int64_t)glist[c] : g0 + c;
}

template <typename XT>
__global__ __launch_bounds__(256) void k_nx_fill_dense(const XT* __restrict__ X, int64_t n, int64_t G,
                                                       const int32_t* __restrict__ glist, int64_t g0, int w, int TW,
                                                       const int64_t* __restrict__ orig, const double* __restrict__ colsum,
                                                       double* __restrict__ t) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n * TW) return;
  const int64_t i = k / TW;
  const int c = (int)(k - i * TW);
  double v = 0.0;
  if (c < w) {
    int64_t o = orig ? orig[i] : i;
    if (o < 0 || o >= n) o = i;          // (cna_set_cell_order has checked the order: never taken)
    v = __ddiv_rn((double)X[o * G + nb_gene(glist, g0, c)], colsum[i]);
  }
  t[k] = v;
}

// grid: (blocks, w); the tile has been cleared: 0 / c = 0
template <typename XT>
__global__ __launch_bounds__(256) void k_nx_fill_lists(const int64_t* __restrict__ gptr, const int32_t* __restrict__ gcell,
                                                       const XT* __restrict__ gval, const int32_t* __restrict__ glist,
                                                       int64_t g0, int TW, int64_t n, const int32_t* __restrict__ inv,
                                                       const double* __restrict__ colsum, double* __restrict__ t) {
  const int c = blockIdx.y;
  const int64_t g = nb_gene(glist, g0, c);
  const int64_t lo = gptr[g], hi = gptr[g + 1];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < hi; e += stride) {
    const int64_t cell = gcell[e];
    if (cell < 0 || cell >= n) continue;   // (the upload has checked the cells: never taken)
    const int64_t i = inv[cell];
    t[i * TW + c] = __ddiv_rn((double)gval[e], colsum[i]);
  }
}

__global__ __launch_bounds__(256) void k_nx_fill_ones(const double* __restrict__ colsum, int64_t n, int TW,
                                                      double* __restrict__ t) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n * TW) return;
  const int64_t i = k / TW;
  t[k] = (k - i * TW) == 0 ? __ddiv_rn(1.0, colsum[i]) : 0.0;
}

// One step on a tile.  A wave owns 64 / TW consecutive rows; a lane is one column of one of them and adds the row's
// entries in stored order.  NB_U neighbour rows are requested together and added one by one; in the last, partial batch
// of a row the missing requests go to the row's own state (wanted next anyway) and are never added.
template <typename VT, int TW, bool LAST>
__global__ __launch_bounds__(256) void k_nx_step(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                 const VT* __restrict__ val, const double* __restrict__ colsum,
                                                 const double* __restrict__ tin, double* __restrict__ tout, int64_t n, int w,
                                                 double self_w, int chunk) {
  constexpr int R = 64 / TW;
  const int lane = threadIdx.x & 63;
  // workgroup -> rows as in the dense walk (diffuse.hip: my_row): the workgroups with blockIdx % 8 == x take `chunk`
  // consecutive blocks of rows at a time, so that the neighbour rows one XCD gathers stay in its L2 (a pure speed choice)
  const int64_t b = blockIdx.x >> 3, x = blockIdx.x & 7;
  const int64_t blk = (b / chunk) * (8 * (int64_t)chunk) + x * chunk + (b % chunk);
  const int64_t wave = blk * 4 + (threadIdx.x >> 6);
  int64_t row = wave * R + lane / TW;
  if (R == 1) row = uniform64(row);
  const int col = lane % TW;
  if (row >= n || col >= w) return;
  int64_t e = indptr[row];
  int64_t end = indptr[row + 1];
  if (R == 1) {
    e = uniform64(e);
    end = uniform64(end);
  }
  const double* __restrict__ tc = tin + col;
  double acc = 0.0;
  for (; e < end; e += NB_U) {
    int64_t j[NB_U];
    double a[NB_U], t[NB_U];
#pragma unroll
    for (int u = 0; u < NB_U; ++u) {
      const bool ok = e + u < end;
      j[u] = ok ? (int64_t)idx[e + u] : row;
      a[u] = ok ? (double)val[e + u] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < NB_U; ++u) t[u] = tc[j[u] * TW];
#pragma unroll
    for (int u = 0; u < NB_U; ++u)
      if (e + u < end) acc = acc + a[u] * t[u];
  }
  const double s = acc + self_w * tc[row * TW];
  tout[row * TW + col] = LAST ? s : __ddiv_rn(s, colsum[row]);
}

// out[(orig ? orig[i] : i) * ld + c] = t[i][c], c < w
__global__ __launch_bounds__(256) void k_nx_unpermute(const double* __restrict__ t, int64_t n, int TW, int w,
                                                      const int64_t* __restrict__ orig, double* __restrict__ out, int ld) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n * w) return;
  const int64_t i = k / w;
  const int c = (int)(k - i * w);
  int64_t o = orig ? orig[i] : i;
  if (o < 0 || o >= n) return;
  out[o * ld + c] = t[i * TW + c];
}

// ------------------------------------------------------------------ keys
__global__ __launch_bounds__(256) void k_nx_keys(const double* __restrict__ V, int64_t n, int q, const int64_t* __restrict__ orig,
                                                 const double* __restrict__ den, double* __restrict__ vdev) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  int64_t o = orig ? orig[i] : i;
  const bool good = nb_good(den[i]) && o >= 0 && o < n;
  for (int j = 0; j < q; ++j) vdev[(int64_t)j * n + i] = good ? V[(int64_t)j * n + o] : nan;
}

__global__ __launch_bounds__(256) void k_nx_keytab(const double* __restrict__ vdev, int64_t n, int q, int Q,
                                                   const double* __restrict__ ks, double* __restrict__ tab,
                                                   uint32_t* __restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t m = 0;
  for (int j = 0; j < Q; ++j) {
    double vc = 0.0;
    if (j < q) {
      const double x = vdev[(int64_t)j * n + i];
      if (finite_d(x)) {
        vc = x - ks[j * KS_LD + 1];
        m |= 1u << j;
      }
    }
    tab[i * Q + j] = vc;
  }
  mask[i] = m;
}

// ------------------------------------------------------------------ moments
// A slab of rows belongs to one group of TW lanes (64 / TW slabs per wave); slab s covers the rows
// [s * slab_rows, (s + 1) * slab_rows).  NB_U rows are requested together and added one by one, in row order.  The partial
// sums are stored slab-minor -- part[(field * TW + column) * nslab + slab] -- so that the fold reads them coalesced.
// part1[j][c][s] = sum of m over the slab's cells of key j
template <int Q, int TW>
__global__ __launch_bounds__(256) void k_nx_pass1(double* __restrict__ t, const double* __restrict__ den,
                                                  const uint32_t* __restrict__ mask, int64_t n, int w, int64_t slab_rows,
                                                  int64_t nslab, double* __restrict__ part) {
  constexpr int R = 64 / TW;
  const int lane = threadIdx.x & 63;
  const int64_t slab = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * R + lane / TW;
  const int col = lane % TW;
  if (slab >= nslab || col >= w) return;
  const int64_t r0 = slab * slab_rows;
  const int64_t r1 = r0 + slab_rows < n ? r0 + slab_rows : n;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double sm[Q];
#pragma unroll
  for (int j = 0; j < Q; ++j) sm[j] = 0.0;
  for (int64_t r = r0; r < r1; r += NB_U) {
    double s[NB_U], d[NB_U];
    uint32_t mk[NB_U];
#pragma unroll
    for (int u = 0; u < NB_U; ++u) {
      const int64_t rr = r + u < r1 ? r + u : r1 - 1;
      s[u] = t[rr * TW + col];
      d[u] = den[rr];
      mk[u] = mask[rr];
    }
#pragma unroll
    for (int u = 0; u < NB_U; ++u) {
      if (r + u < r1) {
        const double m = nb_good(d[u]) ? __ddiv_rn(s[u], d[u]) : nan;
        t[(r + u) * TW + col] = m;
#pragma unroll
        for (int j = 0; j < Q; ++j)
          if (mk[u] >> j & 1) sm[j] += m;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < Q; ++j) part[((int64_t)j * TW + col) * nslab + slab] = sm[j];
}

// the partial sums of one (field, column) added in a fixed order: lane l adds the slabs l, l + 64, ... in turn, then the
// wave's fixed tree -- the same bits on every run
__device__ __forceinline__ double nx_fold(const double* __restrict__ p, int64_t nslab, int lane) {
  double s = 0.0;
  for (int64_t k = lane; k < nslab; k += 64) s += p[k];
  return wave_sum(s);
}

// one wave per (key, column): mean[j][c] = (sum over the slabs) / n_j
__global__ __launch_bounds__(256) void k_nx_mean(const double* __restrict__ part, int64_t nslab, int Q, int TW,
                                                 const double* __restrict__ ks, double* __restrict__ mean) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= Q * TW) return;
  const double s = nx_fold(part + (int64_t)k * nslab, nslab, lane);
  if (lane == 0) mean[k] = s / ks[(k / TW) * KS_LD];
}

// part2[j][c][s] = sum (m - mean)^2, part2[Q + j][c][s] = sum (m - mean)(v_j - mean v_j)
template <int Q, int TW>
__global__ __launch_bounds__(256) void k_nx_pass2(const double* __restrict__ t, const double* __restrict__ tab,
                                                  const uint32_t* __restrict__ mask, const double* __restrict__ mean, int64_t n,
                                                  int w, int64_t slab_rows, int64_t nslab, double* __restrict__ part) {
  constexpr int R = 64 / TW;
  const int lane = threadIdx.x & 63;
  const int64_t slab = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * R + lane / TW;
  const int col = lane % TW;
  if (slab >= nslab || col >= w) return;
  const int64_t r0 = slab * slab_rows;
  const int64_t r1 = r0 + slab_rows < n ? r0 + slab_rows : n;
  double mu[Q], s2[Q], sv[Q];
#pragma unroll
  for (int j = 0; j < Q; ++j) {
    mu[j] = mean[j * TW + col];
    s2[j] = 0.0;
    sv[j] = 0.0;
  }
  for (int64_t r = r0; r < r1; r += NB_U) {
    double m[NB_U];
    uint32_t mk[NB_U];
#pragma unroll
    for (int u = 0; u < NB_U; ++u) {
      const int64_t rr = r + u < r1 ? r + u : r1 - 1;
      m[u] = t[rr * TW + col];
      mk[u] = r + u < r1 ? mask[rr] : 0u;
    }
#pragma unroll
    for (int u = 0; u < NB_U; ++u) {
      if (mk[u] == 0) continue;
      const double* v = tab + (r + u) * Q;
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        if (mk[u] >> j & 1) {
          const double d = m[u] - mu[j];
          s2[j] = fma(d, d, s2[j]);
          sv[j] = fma(d, v[j], sv[j]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < Q; ++j) {
    part[((int64_t)j * TW + col) * nslab + slab] = s2[j];
    part[((int64_t)(Q + j) * TW + col) * nslab + slab] = sv[j];
  }
}

// one wave per (key, column); res: [r | mean | sd], q x G each
__global__ __launch_bounds__(256) void k_nx_finish(const double* __restrict__ part, int64_t nslab, int q, int Q, int TW, int w,
                                                   const double* __restrict__ ks, const double* __restrict__ mean,
                                                   const unsigned char* __restrict__ constant, int64_t g0, int64_t G,
                                                   double* __restrict__ res) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= q * TW) return;
  const int j = k / TW, c = k - j * TW;
  if (c >= w) return;
  const double s2 = nx_fold(part + ((int64_t)j * TW + c) * nslab, nslab, lane);
  const double sv = nx_fold(part + ((int64_t)(Q + j) * TW + c) * nslab, nslab, lane);
  if (lane != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double* kj = ks + j * KS_LD;
  const double N = kj[0];
  const int64_t g = g0 + c;
  double r = nan;
  if (N >= 2.0 && kj[4] < kj[5] && !constant[g]) {
    r = sv / sqrt(s2) / sqrt(kj[2]);
    if (r > 1.0) r = 1.0;
    if (r < -1.0) r = -1.0;
  }
  res[(int64_t)j * G + g] = r;
  res[((int64_t)q + j) * G + g] = N > 0.0 ? mean[j * TW + c] : nan;
  res[(2 * (int64_t)q + j) * G + g] = N > 0.0 ? sqrt(s2 / N) : nan;
}

// ------------------------------------------------------------------ constant genes
// dense: lane = gene, one wave per (64 genes, slab of rows); range[slab][0 / 1][g] = minimum / maximum
template <typename XT>
__global__ __launch_bounds__(64) void k_nx_range_dense(const XT* __restrict__ X, int64_t n, int64_t G, int64_t slab_rows,
                                                       double* __restrict__ range) {
  const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= G) return;
  const int64_t r0 = (int64_t)blockIdx.y * slab_rows;
  const int64_t r1 = r0 + slab_rows < n ? r0 + slab_rows : n;
  XT mn = (XT)INFINITY, mx = (XT)-INFINITY;
  for (int64_t r = r0; r < r1; r += NB_U) {
    XT x[NB_U];
#pragma unroll
    for (int u = 0; u < NB_U; ++u) x[u] = X[(r + u < r1 ? r + u : r1 - 1) * G + g];
#pragma unroll
    for (int u = 0; u < NB_U; ++u) {
      mn = x[u] < mn ? x[u] : mn;
      mx = x[u] > mx ? x[u] : mx;
    }
  }
  range[((int64_t)blockIdx.y * 2) * G + g] = (double)mn;
  range[((int64_t)blockIdx.y * 2 + 1) * G + g] = (double)mx;
}

__global__ __launch_bounds__(256) void k_nx_range_fold(const double* __restrict__ range, int nslab, int64_t G,
                                                       unsigned char* __restrict__ constant) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  double mn = INFINITY, mx = -INFINITY;
  for (int p = 0; p < nslab; ++p) {
    mn = fmin(mn, range[((int64_t)p * 2) * G + g]);
    mx = fmax(mx, range[((int64_t)p * 2 + 1) * G + g]);
  }
  constant[g] = mn == mx ? 1 : 0;
}

// gene-major lists: one wave per gene; a list shorter than the cells holds implicit zeros
template <typename XT>
__global__ __launch_bounds__(256) void k_nx_range_lists(const int64_t* __restrict__ gptr, const XT* __restrict__ gval, int64_t n,
                                                        int64_t G, unsigned char* __restrict__ constant) {
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (g >= G) return;
  const int64_t lo = gptr[g], hi = gptr[g + 1];
  double mn = INFINITY, mx = -INFINITY;
  for (int64_t e = lo + lane; e < hi; e += 64) {
    const double x = (double)gval[e];
    mn = fmin(mn, x);
    mx = fmax(mx, x);
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  if (hi - lo < n) {
    mn = fmin(mn, 0.0);
    mx = fmax(mx, 0.0);
  }
  if (lane == 0) constant[g] = mn == mx ? 1 : 0;
}

// ------------------------------------------------------------------ host side
// what both entries need of the context: a graph held whole by one rank, its column sums, a resident matrix of as many cells
int nb_ready(cna_ctx* c, const char* who, ExprState** es) {
  if (!c->indptr) CNA_FAIL(CNA_ESTATE, std::string(who) + " before cna_graph_upload");
  if (comm_active(c) || c->nranks != 1 || c->local_view || c->n_local != c->n_global)
    CNA_FAIL(CNA_ESTATE, std::string(who) + ": one rank holding the whole graph only (no communicator)");
  if (!c->have_colsum) CNA_FAIL(CNA_ESTATE, std::string(who) + " needs cna_colsums");
  ExprState* s = expr_state(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, std::string(who) + ": no expression matrix is resident (cna_expr_upload_*)");
  if (s->n != c->n_global)
    CNA_FAIL(CNA_EINVAL, std::string(who) + ": the expression matrix has " + std::to_string(s->n) + " cells, the graph " +
                             std::to_string(c->n_global));
  *es = s;
  return 0;
}

int nb_tile_width() {
  const char* e = getenv("CNA_NBHD_TILE");          // experiments (tools/kbench_gene_nbhd_corr.py)
  return e && atoi(e) == 32 ? 32 : 64;
}

// CNA_ENOMEM leaves nothing of the call resident
int nb_need(cna_ctx* c, ExprState* s, NbhdWork* w, std::initializer_list<BufSize> bufs, const char* who) {
  const int rc = result_bufs_need(c, s->st, bufs);
  if (rc == CNA_ENOMEM) {
    (void)hipStreamSynchronize(s->st);
    bufs_free(c, *w);
    cna_set_error(std::string(who) + ": the tile buffers do not fit on the device; nothing of the call is resident");
  }
  return rc;
}

unsigned nb_blocks(int64_t items) { return (unsigned)((items + 255) / 256); }

struct Tile {
  const int32_t* glist;   // device: the genes of the columns, or null: g0 + column
  int64_t g0;
  int w;
};

void nb_fill(cna_ctx* c, ExprState* s, NbhdWork* w, const Tile& t, int TW, double* dst) {
  const int64_t n = s->n;
  const int64_t* orig = (const int64_t*)c->orig_idx;
  with_bool(s->is_f64 != 0, [&](auto f64) {
    using XT = std::conditional_t<decltype(f64)::value, double, float>;
    if (s->format == 1) {
      hipLaunchKernelGGL(k_nx_fill_dense<XT>, dim3(nb_blocks(n * TW)), dim3(256), 0, s->st, s->X.as<const XT>(), n, s->G, t.glist,
                         t.g0, t.w, TW, orig, (const double*)c->colsum, dst);
    } else {
      (void)hipMemsetAsync(dst, 0, (size_t)(8 * n * TW), s->st);
      const unsigned nb = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, (s->nnz / std::max<int64_t>(1, s->G) + 255) / 256));
      hipLaunchKernelGGL(k_nx_fill_lists<XT>, dim3(nb, (unsigned)t.w), dim3(256), 0, s->st, s->gptr.as<const int64_t>(),
                         s->gcell.as<const int32_t>(), s->gval.as<const XT>(), t.glist, t.g0, TW, n, w->inv.as<const int32_t>(),
                         (const double*)c->colsum, dst);
    }
  });
}

// nsteps steps from w->ta; returns the tile that holds the unscaled state
double* nb_walk(cna_ctx* c, ExprState* s, NbhdWork* w, int TW, int width, int nsteps) {
  const int64_t n = s->n;
  double* cur = w->ta.as<double>();
  double* nxt = w->tb.as<double>();
  const int R = 64 / TW;
  // 128 workgroups = one cluster of the device order per XCD at a time (diffuse.hip: step_xcd_chunk); CNA_NBHD_XCD=0:
  // blocks of rows dealt round-robin (experiments: tools/kbench_gene_nbhd_corr.py)
  const int64_t nblk = (n + 4 * R - 1) / (4 * R);
  int64_t cpx = (nblk + 7) / 8;
  const char* e = getenv("CNA_NBHD_XCD");
  const int64_t chunk = e && atoi(e) == 0 ? 1 : std::min<int64_t>(128, cpx);
  cpx = (cpx + chunk - 1) / chunk * chunk;      // whole chunks per XCD
  const dim3 grid((unsigned)(cpx * 8));
  for (int k = 0; k < nsteps; ++k) {
    const bool last = k == nsteps - 1;
    with_bool(c->data_f64 != 0, [&](auto f64) {
      using VT = std::conditional_t<decltype(f64)::value, double, float>;
      with_bool(last, [&](auto l) {
        constexpr bool L = decltype(l)::value;
        if (TW == 64)
          hipLaunchKernelGGL((k_nx_step<VT, 64, L>), grid, dim3(256), 0, s->st, (const int64_t*)c->indptr,
                             (const int32_t*)c->indices, (const VT*)c->data, (const double*)c->colsum, (const double*)cur, nxt, n,
                             width, c->self_weight, (int)chunk);
        else
          hipLaunchKernelGGL((k_nx_step<VT, 32, L>), grid, dim3(256), 0, s->st, (const int64_t*)c->indptr,
                             (const int32_t*)c->indices, (const VT*)c->data, (const double*)c->colsum, (const double*)cur, nxt, n,
                             width, c->self_weight, (int)chunk);
      });
    });
    std::swap(cur, nxt);
  }
  return cur;
}

// the tiles, the inverse order for the lists, the denominator (device order) in w->den
int nb_begin(cna_ctx* c, ExprState* s, NbhdWork* w, int TW, int nsteps, const char* who) {
  const int64_t n = s->n;
  CNA_TRY(nb_need(c, s, w, {{&w->ta, 8 * n * TW}, {&w->tb, 8 * n * TW}, {&w->den, 8 * n}, {&w->inv, 4 * n}}, who));
  // whatever the main stream has queued on the graph, its order and the column sums comes first
  HIP_TRY(hipEventRecord(s->x_ready, c->stream));
  HIP_TRY(hipStreamWaitEvent(s->st, s->x_ready, 0));
  if (s->format == 2)
    hipLaunchKernelGGL(k_nx_inverse, dim3(nb_blocks(n)), dim3(256), 0, s->st, (const int64_t*)c->orig_idx, n, w->inv.as<int32_t>());
  hipLaunchKernelGGL(k_nx_fill_ones, dim3(nb_blocks(n * TW)), dim3(256), 0, s->st, (const double*)c->colsum, n, TW,
                     w->ta.as<double>());
  const double* ones = nb_walk(c, s, w, TW, 1, nsteps);
  hipLaunchKernelGGL(k_nx_unpermute, dim3(nb_blocks(n)), dim3(256), 0, s->st, ones, n, TW, 1, (const int64_t*)nullptr,
                     w->den.as<double>(), 1);
  HIP_TRY(hipGetLastError());
  return 0;
}

double nb_ms(hipStream_t st, std::chrono::steady_clock::time_point& t0) {
  (void)hipStreamSynchronize(st);
  const auto t1 = std::chrono::steady_clock::now();
  const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
  t0 = t1;
  return ms;
}

}  // namespace

extern "C" int cna_nbhd_expr(cna_ctx* c, const int32_t* genes, int m, int nsteps, double* num_out, double* den_out) {
  CHECK_CTX(c);
  ExprState* s = nullptr;
  CNA_TRY(nb_ready(c, "cna_nbhd_expr", &s));
  if (!genes || !num_out || !den_out) CNA_FAIL(CNA_EINVAL, "cna_nbhd_expr: null pointer");
  if (m < 1 || m > NB_MAX_GENES) CNA_FAIL(CNA_EINVAL, "cna_nbhd_expr: 1 <= m <= 64 genes");
  if (nsteps < 1 || nsteps > NB_MAX_STEPS) CNA_FAIL(CNA_EINVAL, "cna_nbhd_expr: 1 <= nsteps <= 15");
  for (int k = 0; k < m; ++k)
    if (genes[k] < 0 || genes[k] >= s->G) CNA_FAIL(CNA_EINVAL, "cna_nbhd_expr: a gene lies outside [0, n_genes)");
  const int64_t n = s->n;
  const int TW = 64;
  NbhdWork* w = expr_work<NbhdWork>(s, EXPR_NBHD);
  CNA_TRY(nb_need(c, s, w, {{&w->glist, 4 * NB_MAX_GENES}, {&w->out, 8 * n * (m + 1)}}, "cna_nbhd_expr"));
  CNA_TRY(nb_begin(c, s, w, TW, nsteps, "cna_nbhd_expr"));
  HIP_TRY(hipMemcpyAsync(w->glist.p, genes, (size_t)(4 * m), hipMemcpyHostToDevice, s->st));
  const Tile tile{w->glist.as<const int32_t>(), 0, m};
  nb_fill(c, s, w, tile, TW, w->ta.as<double>());
  const double* num = nb_walk(c, s, w, TW, m, nsteps);
  double* out = w->out.as<double>();
  const int64_t* orig = (const int64_t*)c->orig_idx;
  hipLaunchKernelGGL(k_nx_unpermute, dim3(nb_blocks(n * m)), dim3(256), 0, s->st, num, n, TW, m, orig, out, m);
  hipLaunchKernelGGL(k_nx_unpermute, dim3(nb_blocks(n)), dim3(256), 0, s->st, w->den.as<const double>(), n, 1, 1, orig,
                     out + n * m, 1);
  return fetch_results(s->st, "cna_nbhd_expr",
                       {{num_out, out, (size_t)(8 * n * m)}, {den_out, out + n * m, (size_t)(8 * n)}});
}

extern "C" int cna_gene_nbhd_corr(cna_ctx* c, const double* V, int q, int nsteps, double* r_out, double* mean_out,
                                  double* sd_out, int64_t* n_cells_out, double* times_ms_out) {
  CHECK_CTX(c);
  ExprState* s = nullptr;
  CNA_TRY(nb_ready(c, "cna_gene_nbhd_corr", &s));
  if (!V || !r_out || !mean_out || !sd_out || !n_cells_out) CNA_FAIL(CNA_EINVAL, "cna_gene_nbhd_corr: null pointer");
  if (q < 1 || q > NB_MAXQ) CNA_FAIL(CNA_EINVAL, "cna_gene_nbhd_corr: 1 <= q <= 16 key columns");
  if (nsteps < 1 || nsteps > NB_MAX_STEPS) CNA_FAIL(CNA_EINVAL, "cna_gene_nbhd_corr: 1 <= nsteps <= 15");
  int Q = 1;
  while (Q < q) Q *= 2;
  const int64_t n = s->n, G = s->G;
  const int TW = nb_tile_width();
  const int R = 64 / TW;
  const int64_t slab_rows = std::max<int64_t>(NB_MIN_SLAB, (n + NB_SLABS - 1) / NB_SLABS);
  const int64_t nslab = (n + slab_rows - 1) / slab_rows;
  const int range_slabs = (int)std::max<int64_t>(1, std::min<int64_t>(NB_RANGE_SLABS, n / 64));
  const int64_t range_rows = (n + range_slabs - 1) / range_slabs;
  NbhdWork* w = expr_work<NbhdWork>(s, EXPR_NBHD);
  hipStream_t st = s->st;
  CNA_TRY(nb_need(c, s, w,
                  {{&w->vraw, 8 * n * q}, {&w->vdev, 8 * n * q}, {&w->vtab, 8 * n * Q}, {&w->vmask, 4 * n},
                   {&w->kstat, 8 * KS_LD * NB_MAXQ}, {&w->part, 8 * nslab * 2 * Q * TW}, {&w->mean, 8 * Q * TW},
                   {&w->range, s->format == 1 ? 8 * 2 * (int64_t)range_slabs * G : 256}, {&w->flag, G}, {&w->res, 8 * 3 * q * G}},
                  "cna_gene_nbhd_corr"));
  auto t0 = std::chrono::steady_clock::now();
  double t_fill = 0, t_step = 0, t_mom = 0;
  const bool timed = times_ms_out != nullptr;
  if (timed) (void)nb_ms(st, t0);
  CNA_TRY(nb_begin(c, s, w, TW, nsteps, "cna_gene_nbhd_corr"));
  if (timed) t_step += nb_ms(st, t0);
  // the keys in the device's order, their statistics over the cells with a good denominator, the centred table
  HIP_TRY(hipMemcpyAsync(w->vraw.p, V, (size_t)(8 * n * q), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_nx_keys, dim3(nb_blocks(n)), dim3(256), 0, st, w->vraw.as<const double>(), n, q,
                     (const int64_t*)c->orig_idx, w->den.as<const double>(), w->vdev.as<double>());
  hipLaunchKernelGGL(k_key_stats, dim3(q), dim3(1024), 0, st, w->vdev.as<const double>(), n, w->kstat.as<double>());
  hipLaunchKernelGGL(k_nx_keytab, dim3(nb_blocks(n)), dim3(256), 0, st, w->vdev.as<const double>(), n, q, Q,
                     w->kstat.as<const double>(), w->vtab.as<double>(), w->vmask.as<uint32_t>());
  // constant genes, over all cells of the raw matrix
  with_bool(s->is_f64 != 0, [&](auto f64) {
    using XT = std::conditional_t<decltype(f64)::value, double, float>;
    if (s->format == 1) {
      hipLaunchKernelGGL(k_nx_range_dense<XT>, dim3((unsigned)((G + 63) / 64), (unsigned)range_slabs), dim3(64), 0, st,
                         s->X.as<const XT>(), n, G, range_rows, w->range.as<double>());
      hipLaunchKernelGGL(k_nx_range_fold, dim3(nb_blocks(G)), dim3(256), 0, st, w->range.as<const double>(), range_slabs, G,
                         w->flag.as<unsigned char>());
    } else {
      hipLaunchKernelGGL(k_nx_range_lists<XT>, dim3((unsigned)((G + 3) / 4)), dim3(256), 0, st, s->gptr.as<const int64_t>(),
                         s->gval.as<const XT>(), n, G, w->flag.as<unsigned char>());
    }
  });
  HIP_TRY(hipGetLastError());
  if (timed) t_mom += nb_ms(st, t0);
  const dim3 mgrid((unsigned)((nslab + 4 * R - 1) / (4 * R)));
  for (int64_t g0 = 0; g0 < G; g0 += TW) {
    const int width = (int)std::min<int64_t>(TW, G - g0);
    const Tile tile{nullptr, g0, width};
    nb_fill(c, s, w, tile, TW, w->ta.as<double>());
    if (timed) t_fill += nb_ms(st, t0);
    double* num = nb_walk(c, s, w, TW, width, nsteps);
    if (timed) t_step += nb_ms(st, t0);
    with_width(Q, [&](auto width_c) {
      constexpr int QQ = decltype(width_c)::value;
      with_bool(TW == 64, [&](auto wide) {
        constexpr int TT = decltype(wide)::value ? 64 : 32;
        hipLaunchKernelGGL((k_nx_pass1<QQ, TT>), mgrid, dim3(256), 0, st, num, w->den.as<const double>(),
                           w->vmask.as<const uint32_t>(), n, width, slab_rows, nslab, w->part.as<double>());
        hipLaunchKernelGGL(k_nx_mean, dim3((unsigned)((QQ * TT + 3) / 4)), dim3(256), 0, st, w->part.as<const double>(), nslab, QQ, TT,
                           w->kstat.as<const double>(), w->mean.as<double>());
        hipLaunchKernelGGL((k_nx_pass2<QQ, TT>), mgrid, dim3(256), 0, st, (const double*)num, w->vtab.as<const double>(),
                           w->vmask.as<const uint32_t>(), w->mean.as<const double>(), n, width, slab_rows, nslab,
                           w->part.as<double>());
      });
    });
    hipLaunchKernelGGL(k_nx_finish, dim3((unsigned)((q * TW + 3) / 4)), dim3(256), 0, st, w->part.as<const double>(), nslab, q, Q, TW, width,
                       w->kstat.as<const double>(), w->mean.as<const double>(), w->flag.as<const unsigned char>(), g0, G,
                       w->res.as<double>());
    HIP_TRY(hipGetLastError());
    if (timed) t_mom += nb_ms(st, t0);
  }
  double ks_h[KS_LD * NB_MAXQ];
  const double* res = w->res.as<const double>();
  const size_t rb = (size_t)(8 * q * G);
  CNA_TRY(fetch_results(st, "cna_gene_nbhd_corr",
                        {{r_out, res, rb}, {mean_out, res + q * G, rb}, {sd_out, res + 2 * q * G, rb},
                         {ks_h, w->kstat.p, sizeof(double) * KS_LD * (size_t)q}}));
  for (int j = 0; j < q; ++j) n_cells_out[j] = (int64_t)ks_h[j * KS_LD];
  if (timed) {
    times_ms_out[0] = t_fill;
    times_ms_out[1] = t_step;
    times_ms_out[2] = t_mom;
  }
  return 0;
}

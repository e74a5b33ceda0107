// The neighbourhood coefficient by cluster (cna.tl.coef_strata): the numbers behind the reference's
//     sc.tl.leiden(d); cna.pl.violinplot(d, 'leiden', key='coef')            (demo/demo.ipynb; plotting/_strat.py:21-29)
// per level of a clustering: counts, mean, sum (v - mean)^2, minimum, median, maximum of the coefficient over the cells
// that have one, how many of them pass the FDR with either sign (plotting/_umap.py:10), and the Gaussian kernel density
// on the grid that Axes.violinplot draws (matplotlib.cbook.violin_stats with mlab.GaussianKDE), cna_coef_strata.
//
// Nothing here reads or writes the state of c_api.hip or the resident expression matrix: the three per-cell columns are in
// the CALLER's cell order, the buffers are this entry's own (StrataWork), the stream is the expression stream.
//
//   sort (expr.h)   checks every code against [-1, n_bins); per block of cells and bin: the kept cells (code >= 0, finite
//                   value) for the scan, and the bin's cells / kept cells passing the FDR with v > 0 / v < 0 (integer
//                   atomics, LDS then global); then the kept values, bin after bin, ascending in the cell index inside a bin
//   k_st_mom1/2     per chunk (ST_CHUNK values of one bin's segment): sum, min, max; then sum (v - mean)^2.  k_st_fold1/2
//                   add the partials of a bin in chunk order and derive the bandwidth, the norm and the grid step
//   k_st_hist       one pass of the exact radix select, every bin at once: histogram [bin][rank][256] of the 8-bit digit at
//                   `shift` among the values whose order-preserving key matches the prefix of the lower / upper middle
//                   element; k_st_pick chooses the digit on the device (no host round trip in the eight passes)
//   k_st_density    one wave per chunk, all of the bin's grid points: ceil(points / 64) points and their sums per lane in
//                   registers, the chunk's values staged in LDS and read as broadcasts; per value and point one subtract,
//                   two multiplies and a float64 exp.  One partial per (chunk, point) with plain stores
//   k_st_finish     adds the partials of a (bin, point) in chunk order and divides by the norm; the all-equal fallback
//
// Sums take a fixed order (no floating-point atomics): two runs on one input give the same bits.
#include "expr.h"
#include <cmath>
#include <cstring>

namespace {

constexpr int ST_MAX_BINS = 1024;
constexpr int ST_MAX_POINTS = 1024;
// Values of one bin that one wave of k_st_density takes.  With the software exp the kernel takes 42 VGPRs at two points
// per lane (72 at eight, 112 at sixteen: 8 / 7 / 4 waves per SIMD), so latency is hidden by waves, not by a long chunk:
// 512 values leave 2M cells ~4000 waves, four per SIMD of the 256 CUs, stage 4 KB of LDS per wave, and keep the partials
// (chunks x points doubles) at 1/512 of the work.
constexpr int64_t ST_CHUNK = 512;
constexpr int BS_LD = 8;   // doubles per bin: mean, ssd, min, median, max, grid step, inv / 2, norm

// the sort's policy: a cell with a code >= 0 is kept when its value is finite, what is stored is the value; tallies 1 to 3:
// the bin's cells, its kept cells passing the FDR with v > 0, with v < 0
struct KeptValues {
  static constexpr int MAX_BINS = ST_MAX_BINS, TALLIES = 4;
  using payload = double;
  const double* v;
  const double* fdr;               // may be null
  double thresh;
  __device__ double load(int64_t i) const { return v[i]; }
  __device__ bool keep(double x) const { return finite_d(x); }
  __device__ __forceinline__ void tally(unsigned int (*h)[MAX_BINS], int32_t cd, int64_t i, double x, bool kept) const {
    atomicAdd(&h[1][cd], 1u);
    if (kept && fdr && fdr[i] <= thresh) {          // a NaN fdr fails the test
      if (x > 0.0) atomicAdd(&h[2][cd], 1u);
      else if (x < 0.0) atomicAdd(&h[3][cd], 1u);
    }
  }
};

struct StrataWork : BufSet {
  // the value and fdr columns; the sort with the codes, the totals [kept | n | pos | neg] x bins and the chunk table
  // [bptr | first chunk of every bin | {bin, lo, hi} of every chunk]; the kept values by bin
  Buf v{*this}, fdr{*this};
  CodeSort sort{*this};
  Buf seg{*this};
  // per-chunk partials; per-bin block; select state; digit histograms; density partials; the densities
  Buf mom{*this}, bin{*this}, sel{*this}, hist{*this}, part{*this}, vals{*this};
};

__device__ __forceinline__ unsigned long long order_key(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);       // negatives reversed, positives above them
}
__device__ __forceinline__ double key_value(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// np.linspace(mn, mx, points)[j]: j * step + mn in two roundings, the last point mx itself (a single point is mn)
__device__ __forceinline__ double grid_point(double mn, double mx, double step, int j, int points) {
#pragma clang fp contract(off)
  if (j > 0 && j == points - 1) return mx;
  const double t = (double)j * step;
  return t + mn;
}

// ------------------------------------------------------------------ moments
// chunk table: tab[3 ch] = bin, tab[3 ch + 1], tab[3 ch + 2] = the chunk's span of seg (never empty, at most ST_CHUNK).
// Lane l adds the values l, l + 64, ... of the chunk, the 64 sums are folded by wave_sum: a fixed order.
__global__ __launch_bounds__(64) void k_st_mom1(const double* __restrict__ seg, const int64_t* __restrict__ tab, double* __restrict__ mom) {
  const int64_t ch = blockIdx.x, lo = tab[3 * ch + 1], hi = tab[3 * ch + 2];
  double s = 0.0, mn = INFINITY, mx = -INFINITY;
  for (int64_t e = lo + threadIdx.x; e < hi; e += 64) {
    const double x = seg[e];
    s += x;
    mn = fmin(mn, x);
    mx = fmax(mx, x);
  }
  s = wave_sum(s);
  mn = wave_min(mn);
  mx = wave_max(mx);
  if (threadIdx.x == 0) {
    mom[4 * ch] = s;
    mom[4 * ch + 1] = mn;
    mom[4 * ch + 2] = mx;
  }
}

__global__ __launch_bounds__(256) void k_st_fold1(const double* __restrict__ mom, const int64_t* __restrict__ first,
                                                  const unsigned long long* __restrict__ kept, int n_bins, double* __restrict__ bin) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_bins) return;
  double s = 0.0, mn = INFINITY, mx = -INFINITY;
  for (int64_t ch = first[b]; ch < first[b + 1]; ++ch) {
    s += mom[4 * ch];
    mn = fmin(mn, mom[4 * ch + 1]);
    mx = fmax(mx, mom[4 * ch + 2]);
  }
  const unsigned long long m = kept[b];
  double* o = bin + (int64_t)b * BS_LD;
  o[0] = m ? s / (double)m : NAN;
  o[2] = m ? mn : NAN;
  o[4] = m ? mx : NAN;
}

__global__ __launch_bounds__(64) void k_st_mom2(const double* __restrict__ seg, const int64_t* __restrict__ tab,
                                                const double* __restrict__ bin, double* __restrict__ mom) {
  const int64_t ch = blockIdx.x, lo = tab[3 * ch + 1], hi = tab[3 * ch + 2];
  const double mean = bin[tab[3 * ch] * BS_LD];
  double s = 0.0;
  for (int64_t e = lo + threadIdx.x; e < hi; e += 64) {
    const double d = seg[e] - mean;
    s += d * d;
  }
  s = wave_sum(s);
  if (threadIdx.x == 0) mom[4 * ch + 3] = s;
}

struct SelState {
  unsigned long long prefix[2];   // key prefix of the lower / upper middle element so far
  unsigned long long rank[2];     // its rank among the values that share the prefix
};

// ssd, then what the density needs (mlab.GaussianKDE in its own order): var = ssd / (m - 1), the bandwidth factor f,
// inv = (1 / var) / f^2 (stored halved: energy = d * (inv * d) / 2), norm = sqrt(2 pi var f^2) * m, and the grid step.
// bw_kind 0: Scott m^-0.2, 1: Silverman (3 m / 4)^-0.2, 2: bw_value itself.
__global__ __launch_bounds__(256) void k_st_fold2(const double* __restrict__ mom, const int64_t* __restrict__ first,
                                                  const unsigned long long* __restrict__ kept, int n_bins, int points, int bw_kind,
                                                  double bw_value, double* __restrict__ bin, SelState* __restrict__ sel) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_bins) return;
  double s = 0.0;
  for (int64_t ch = first[b]; ch < first[b + 1]; ++ch) s += mom[4 * ch + 3];
  const unsigned long long m = kept[b];
  double* o = bin + (int64_t)b * BS_LD;
  o[1] = m ? s : NAN;
  o[3] = NAN;
  const double dm = (double)m;
  const double var = s / (dm - 1.0);
  const double f = bw_kind == 0 ? pow(dm, -0.2) : (bw_kind == 1 ? pow(dm * 3.0 / 4.0, -0.2) : bw_value);
  const double inv = (1.0 / var) / (f * f);
  o[5] = points > 1 ? (o[4] - o[2]) / (double)(points - 1) : 0.0;
  o[6] = 0.5 * inv;
  o[7] = sqrt(2.0 * 3.141592653589793 * (var * (f * f))) * dm;
  sel[b].prefix[0] = sel[b].prefix[1] = 0ull;
  sel[b].rank[0] = m ? (m - 1) / 2 : 0ull;
  sel[b].rank[1] = m / 2;
}

// ------------------------------------------------------------------ median: exact radix select, every bin at once
__global__ __launch_bounds__(64) void k_st_hist(const double* __restrict__ seg, const int64_t* __restrict__ tab,
                                                const SelState* __restrict__ sel, int shift, unsigned int* __restrict__ hist) {
  __shared__ unsigned int h[2][256];
  for (int i = threadIdx.x; i < 512; i += 64) (&h[0][0])[i] = 0u;
  __syncthreads();
  const int64_t ch = blockIdx.x, b = tab[3 * ch], lo = tab[3 * ch + 1], hi = tab[3 * ch + 2];
  const unsigned long long p0 = sel[b].prefix[0], p1 = sel[b].prefix[1];
  for (int64_t e = lo + threadIdx.x; e < hi; e += 64) {
    const unsigned long long k = order_key(seg[e]);
    const unsigned long long up = shift == 56 ? 0ull : k >> (shift + 8);
    const unsigned d = (unsigned)(k >> shift) & 255u;
    if (up == p0) atomicAdd(&h[0][d], 1u);
    if (up == p1) atomicAdd(&h[1][d], 1u);
  }
  __syncthreads();
  unsigned int* out = hist + b * 512;
  for (int i = threadIdx.x; i < 512; i += 64) {
    const unsigned int t = (&h[0][0])[i];
    if (t) atomicAdd(out + i, t);
  }
}

// one wave per bin: the digit in which each of the two ranks falls (lane l holds the digits 4 l .. 4 l + 3, a prefix sum
// over the lanes finds the one that holds the rank), the histogram left zeroed for the next pass; after the last digit the
// median as np.median forms it: the middle value of an odd count, (lower + upper) / 2 of an even one
__global__ __launch_bounds__(64) void k_st_pick(unsigned int* __restrict__ hist, SelState* __restrict__ sel,
                                                const unsigned long long* __restrict__ kept, int shift, double* __restrict__ bin) {
  const int b = blockIdx.x, lane = threadIdx.x;
  uint4* h = (uint4*)(hist + (int64_t)b * 512);
  if (kept[b]) {                                   // the same in every lane
    unsigned long long pre[2];
    for (int r = 0; r < 2; ++r) {
      const uint4 q = h[r * 64 + lane];
      const unsigned int cs[4] = {q.x, q.y, q.z, q.w};
      const unsigned int own = q.x + q.y + q.z + q.w;
      unsigned int inc = own;
      for (int w = 1; w < 64; w <<= 1) {
        const unsigned int t = __shfl_up(inc, w, 64);
        if (lane >= w) inc += t;
      }
      const unsigned int rank = (unsigned int)sel[b].rank[r];
      const unsigned long long hit = __ballot(rank < inc);
      const int src = hit ? __ffsll((long long)hit) - 1 : 63;
      unsigned int rem = rank - (inc - own);
      int d = 0;
      for (; d < 3; ++d) {
        if (rem < cs[d]) break;
        rem -= cs[d];
      }
      const int digit = __shfl(4 * lane + d, src, 64);
      rem = __shfl(rem, src, 64);
      pre[r] = (sel[b].prefix[r] << 8) | (unsigned long long)digit;
      if (lane == 0) {
        sel[b].prefix[r] = pre[r];
        sel[b].rank[r] = rem;
      }
    }
    if (shift == 0 && lane == 0) {                 // an odd count: the middle value itself (x + x overflows from DBL_MAX / 2 on)
      const double lo = key_value(pre[0]), hi = key_value(pre[1]);
      bin[(int64_t)b * BS_LD + 3] = (kept[b] & 1ull) ? lo : (lo + hi) / 2.0;
    }
  }
  h[lane] = make_uint4(0u, 0u, 0u, 0u);
  h[64 + lane] = make_uint4(0u, 0u, 0u, 0u);
}

// ------------------------------------------------------------------ density
// One wave per chunk.  Lane l holds the grid points l, l + 64, ... (NP of them, those at or past `points` idle) and their
// sums; every value of the chunk is read from LDS by all lanes at once (one address: a broadcast).  A bin whose values are
// all equal (min == max, decided exactly) takes matplotlib's fallback in k_st_finish and is skipped here.
template <int NP>
__global__ __launch_bounds__(64) void k_st_density(const double* __restrict__ seg, const int64_t* __restrict__ tab,
                                                   const double* __restrict__ bin, int points, double* __restrict__ part) {
  __shared__ double sv[ST_CHUNK];
  const int64_t ch = blockIdx.x, lo = tab[3 * ch + 1];
  const int m = (int)(tab[3 * ch + 2] - lo);
  const double* bs = bin + tab[3 * ch] * BS_LD;
  const double mn = bs[2], mx = bs[4], step = bs[5], hinv = bs[6];
  if (!(mn < mx)) return;
  const int lane = threadIdx.x;
  for (int i = lane; i < m; i += 64) sv[i] = seg[lo + i];
  __syncthreads();
  double x[NP], acc[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    x[k] = grid_point(mn, mx, step, lane + 64 * k, points);
    acc[k] = 0.0;
  }
  for (int i = 0; i < m; ++i) {
    const double val = sv[i];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      if (64 * k < points) {                       // wave-uniform
        const double d = val - x[k];
        acc[k] += exp(-(d * (hinv * d)));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NP; ++k)
    if (lane + 64 * k < points) part[ch * points + lane + 64 * k] = acc[k];
}

__global__ __launch_bounds__(256) void k_st_finish(const double* __restrict__ part, const int64_t* __restrict__ first,
                                                   const unsigned long long* __restrict__ kept, const double* __restrict__ bin,
                                                   int n_bins, int points, double* __restrict__ vals) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)n_bins * points) return;
  const int b = (int)(t / points), j = (int)(t % points);
  const double* bs = bin + (int64_t)b * BS_LD;
  double r = 0.0;
  if (kept[b]) {
    const double mn = bs[2], mx = bs[4];
    if (!(mn < mx)) {
      r = grid_point(mn, mx, bs[5], j, points) == mn ? 1.0 : 0.0;      // (X[0] == coords).astype(float)
    } else {
      double s = 0.0;
      for (int64_t ch = first[b]; ch < first[b + 1]; ++ch) s += part[ch * points + j];
      r = s / bs[7];
    }
  }
  vals[t] = r;
}

}  // namespace

extern "C" int cna_coef_strata(cna_ctx* c, const double* v, const double* fdr, const int32_t* codes, int64_t n_cells, int n_bins,
                               int points, int bw_kind, double bw_value, double fdr_thresh, int64_t* n_out, int64_t* n_kept_out,
                               int64_t* n_pos_out, int64_t* n_neg_out, double* mean_out, double* ssd_out, double* min_out,
                               double* median_out, double* max_out, double* vals_out) {
  CHECK_CTX(c);
  if (!v || !codes || !n_out || !n_kept_out || !n_pos_out || !n_neg_out || !mean_out || !ssd_out || !min_out || !median_out ||
      !max_out || !vals_out)
    CNA_FAIL(CNA_EINVAL, "cna_coef_strata: null pointer");
  if (n_cells < 1 || n_cells >= (1ll << 31)) CNA_FAIL(CNA_EINVAL, "cna_coef_strata: cells must lie in [1, 2^31)");
  if (n_bins < 1 || n_bins > ST_MAX_BINS) CNA_FAIL(CNA_EINVAL, "cna_coef_strata: 1 <= n_bins <= 1024");
  if (points < 1 || points > ST_MAX_POINTS) CNA_FAIL(CNA_EINVAL, "cna_coef_strata: 1 <= points <= 1024");
  if (bw_kind < 0 || bw_kind > 2) CNA_FAIL(CNA_EINVAL, "cna_coef_strata: bw_kind is 0 (Scott), 1 (Silverman) or 2 (bw_value)");
  if (bw_kind == 2 && !(bw_value > 0.0 && bw_value <= 1.79769313486231570815e308))
    CNA_FAIL(CNA_EINVAL, "cna_coef_strata: bw_value must be a positive finite number");
  ExprState* es = nullptr;
  CNA_TRY(expr_get_state(c, &es));
  hipStream_t st = es->st;
  StrataWork* s = expr_work<StrataWork>(es, EXPR_STRATA);
  const int64_t n = n_cells;
  CNA_TRY(buf_need(c, st, s->v, 8 * n));
  if (fdr) CNA_TRY(buf_need(c, st, s->fdr, 8 * n));
  HIP_TRY(hipMemcpyAsync(s->v.p, v, (size_t)(8 * n), hipMemcpyHostToDevice, st));
  if (fdr) HIP_TRY(hipMemcpyAsync(s->fdr.p, fdr, (size_t)(8 * n), hipMemcpyHostToDevice, st));
  const KeptValues kept{s->v.as<const double>(), fdr ? s->fdr.as<const double>() : nullptr, fdr_thresh};
  CNA_TRY(sort_count(c, st, s->sort, kept, codes, n, n_bins, ST_CHUNK, 3, "cna_coef_strata: a code lies outside [-1, n_bins)"));
  const std::vector<int64_t>& tot = s->sort.tot_h;
  const int64_t nch = s->sort.nch;
  int64_t kept_all = 0;
  for (int b = 0; b < n_bins; ++b) kept_all += tot[(size_t)b];
  CNA_TRY(buf_need(c, st, s->seg, 8 * std::max<int64_t>(1, kept_all)));
  CNA_TRY(buf_need(c, st, s->mom, 8 * 4 * std::max<int64_t>(1, nch)));
  CNA_TRY(buf_need(c, st, s->bin, 8 * BS_LD * (int64_t)n_bins));
  CNA_TRY(buf_need(c, st, s->sel, (int64_t)sizeof(SelState) * n_bins));
  CNA_TRY(buf_need(c, st, s->hist, 4 * 512 * (int64_t)n_bins));
  CNA_TRY(buf_need(c, st, s->part, 8 * std::max<int64_t>(1, nch) * points));
  CNA_TRY(buf_need(c, st, s->vals, 8 * (int64_t)n_bins * points));
  const unsigned long long* tot_dev = s->sort.totals();
  const int64_t* first = s->sort.first();
  const int64_t* tab = s->sort.chunks();
  double* bin = s->bin.as<double>();
  const unsigned bin_blocks = (unsigned)((n_bins + 255) / 256);
  sort_fill(st, s->sort, kept, n, s->seg.as<double>());
  if (nch) hipLaunchKernelGGL(k_st_mom1, dim3((unsigned)nch), dim3(64), 0, st, (const double*)s->seg.p, tab, (double*)s->mom.p);
  hipLaunchKernelGGL(k_st_fold1, dim3(bin_blocks), dim3(256), 0, st, (const double*)s->mom.p, first, tot_dev, n_bins, bin);
  if (nch) hipLaunchKernelGGL(k_st_mom2, dim3((unsigned)nch), dim3(64), 0, st, (const double*)s->seg.p, tab, (const double*)bin,
                              (double*)s->mom.p);
  hipLaunchKernelGGL(k_st_fold2, dim3(bin_blocks), dim3(256), 0, st, (const double*)s->mom.p, first, tot_dev, n_bins, points, bw_kind,
                     bw_value, bin, (SelState*)s->sel.p);
  HIP_TRY(hipGetLastError());
  if (nch) {
    HIP_TRY(hipMemsetAsync(s->hist.p, 0, (size_t)(4 * 512 * (int64_t)n_bins), st));
    for (int shift = 56; shift >= 0; shift -= 8) {
      hipLaunchKernelGGL(k_st_hist, dim3((unsigned)nch), dim3(64), 0, st, (const double*)s->seg.p, tab, (const SelState*)s->sel.p,
                         shift, (unsigned int*)s->hist.p);
      hipLaunchKernelGGL(k_st_pick, dim3((unsigned)n_bins), dim3(64), 0, st, (unsigned int*)s->hist.p, (SelState*)s->sel.p,
                         tot_dev, shift, bin);
    }
    with_width((points + 63) / 64, [&](auto np) {
      hipLaunchKernelGGL((k_st_density<decltype(np)::value>), dim3((unsigned)nch), dim3(64), 0, st, (const double*)s->seg.p, tab,
                         (const double*)bin, points, (double*)s->part.p);
    });
  }
  hipLaunchKernelGGL(k_st_finish, dim3((unsigned)(((int64_t)n_bins * points + 255) / 256)), dim3(256), 0, st,
                     (const double*)s->part.p, first, tot_dev, (const double*)bin, n_bins, points, (double*)s->vals.p);
  std::vector<double> hb((size_t)BS_LD * n_bins), hv((size_t)n_bins * points);
  CNA_TRY(fetch_results(st, "cna_coef_strata", {{hb.data(), bin, 8 * hb.size()}, {hv.data(), s->vals.p, 8 * hv.size()}}));
  for (int b = 0; b < n_bins; ++b) {
    const double* o = hb.data() + (size_t)b * BS_LD;
    n_kept_out[b] = tot[(size_t)b];
    n_out[b] = tot[(size_t)n_bins + b];
    n_pos_out[b] = tot[2 * (size_t)n_bins + b];
    n_neg_out[b] = tot[3 * (size_t)n_bins + b];
    mean_out[b] = o[0];
    ssd_out[b] = o[1];
    min_out[b] = o[2];
    median_out[b] = o[3];
    max_out[b] = o[4];
  }
  std::memcpy(vals_out, hv.data(), 8 * hv.size());
  return 0;
}

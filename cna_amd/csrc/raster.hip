// The neighbourhood coefficient on the embedding, as images (cna.tl.coef_raster): the numbers behind the reference's
//     cna.pl.umap_ncorr(d, key='case_coef')        (demo/demo.ipynb 1.2, 1.3; plotting/_umap.py:6-36)
//     sc.pl.umap(d, color='NAMPC1', cmap='seismic')                              (demo/demo.ipynb 3.2.1)
// per pixel of a W x H grid over the embedding: the cells that fall into it (the grey layer), and per key the cells that
// PASS (a finite value, and fdr <= fdr_thresh where the key has an fdr), their sum, their largest value (what scanpy's
// sort_order=True leaves on top) and their smallest, cna_coef_raster.
//
// Nothing here reads or writes the state of c_api.hip or the resident expression matrix: the columns are in the CALLER's
// cell order, the buffers are this entry's own (RasterWork), the stream is the expression stream.
//
//   k_rs_extent     automatic extent: min / max of x and of y over the cells where both are finite; wave and workgroup
//                   reduction, then integer atomicMin / atomicMax on the order-preserving key of the double (order-free,
//                   exact), issued only by a workgroup that can still move the value
//   k_rs_pixel      the pixel of every cell by the pixel rule (one subtraction, one multiplication, each rounded on its own),
//                   -1 outside the extent or with a non-finite coordinate; counts the finite cells outside
//   sort (expr.h)   cells -> cell indices sorted by pixel, stable: two passes of the counting sort, low then high
//                   RS_DIGIT_BITS bits of the pixel (up to 2^22 pixels do not fit the LDS of one pass).  Inside a pixel the
//                   cells ascend whatever the scheduling.  k_sort_count and k_sort_fill as they are, on codes made on the
//                   device; the scan over the blocks is k_rs_scan, with 16 loads in flight per thread
//   k_rs_bounds     first and one-past-last position of every pixel in the sorted list, read off where the pixel changes:
//                   no atomics, so a pixel that holds most of the cells costs what any other does
//   k_rs_classify   n per pixel; a pixel with more than RS_SMALL cells is BIG: it is cut into chunks of RS_CHUNK cells
//   k_rs_small      one thread per (pixel, key) with at most RS_SMALL cells: its passing cells in cell order
//   k_rs_chunk      one wave per (chunk of a big pixel, key): lane l adds the cells l, l + 64, ..., folded by wave_sum
//   k_rs_fold       one wave per (big pixel, key): lane l adds the chunk partials l, l + 64, ... in chunk order, wave_sum
//   k_rs_dilate / k_rs_cover   radius > 0: top / bottom / covered over a disc, on the images
//
// Sums take a fixed order (no floating-point atomics): two runs give the same bits.  A dense pixel is spread over
// count / RS_CHUNK waves and neither serialises the call nor changes the order.
#include "expr.h"
#include <cmath>
#include <cstring>
#include <optional>

namespace {

constexpr int RS_MAX_SIDE = 4096, RS_MAX_KEYS = 16, RS_MAX_RADIUS = 16;
constexpr int64_t RS_MAX_PIXELS = 1ll << 22;     // keys x width x height
constexpr int RS_DIGIT_BITS = 11, RS_DIGIT = 1 << RS_DIGIT_BITS;    // 2 x 11 bits hold a pixel; 8 KB of LDS counters
// A pixel with at most RS_SMALL cells is summed by one thread (the common case: 2M cells on 512 x 512 put ~8 in a pixel);
// a larger one by one wave per RS_CHUNK cells, 16 per lane: 2M cells in one pixel are ~2000 waves, 8 per CU.
constexpr int RS_SMALL = 32;
constexpr int RS_CHUNK = 1024;

using RsCells = CellListOf<RS_DIGIT>;            // pass 1: what is stored is the cell index
struct RsPerm {                                   // pass 2: position j of pass 1's list -> the cell stored there
  static constexpr int MAX_BINS = RS_DIGIT, TALLIES = 1;
  using payload = int32_t;
  const int32_t* perm;
  __device__ int32_t load(int64_t j) const { return perm[j]; }
  __device__ bool keep(int32_t) const { return true; }
};

// unsigned long long each, after the 4 extent keys: finite cells outside, chunks, big pixels, and the word k_sort_count flags a
// code outside [-1, n_bins) in (never set: the codes are made here)
enum { RS_C_OUTSIDE = 0, RS_C_SLOTS, RS_C_BIG, RS_C_BAD, RS_COUNTERS };

struct RasterWork : BufSet {
  Buf xy{*this}, v{*this}, fdr{*this};             // the inputs
  Buf pix{*this}, code{*this};                     // pixel of every cell; the digit the current pass sorts by
  Buf cnt{*this}, tot{*this}, bptr{*this};         // the sort: [block][digit] counts, digit totals, digit offsets
  Buf perm1{*this}, perm2{*this};                  // cell indices after pass 1, after pass 2
  Buf range{*this};                                // [pstart | pend], int32 per pixel
  Buf ctr{*this};                                  // 4 extent keys, RS_COUNTERS counters, one absmax key per key
  Buf slot{*this}, big{*this}, part{*this};        // chunks {pixel, index}; big pixels {pixel, first chunk, chunks}; partials
  Buf n_img{*this}, np_img{*this}, sum{*this}, top{*this}, bot{*this}, topr{*this}, botr{*this}, cov{*this};
};

__device__ __forceinline__ unsigned long long rs_order_key(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);       // negatives reversed, positives above them
}
double rs_key_value(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double d;
  std::memcpy(&d, &b, 8);
  return d;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// atomicMax / atomicMin on a value that only rises / falls, behind a plain look at it: a wave that cannot move it does not
// queue on its address (a stale look costs a needless atomic, never a missed one)
__device__ __forceinline__ void rs_raise(unsigned long long* a, unsigned long long k) {
  if (k > __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a, k);
}
__device__ __forceinline__ void rs_lower(unsigned long long* a, unsigned long long k) {
  if (k < __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(a, k);
}

// ------------------------------------------------------------------ extent and pixels
// key[0], key[1] = min, max of x; key[2], key[3] = of y (as order keys; start ~0, 0, ~0, 0)
__global__ __launch_bounds__(256) void k_rs_extent(const double* __restrict__ xy, int64_t n, unsigned long long* __restrict__ key) {
  double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double x = xy[2 * i], y = xy[2 * i + 1];
    if (finite_d(x) && finite_d(y)) {
      x0 = fmin(x0, x); x1 = fmax(x1, x);
      y0 = fmin(y0, y); y1 = fmax(y1, y);
    }
  }
  x0 = wave_min(x0); x1 = wave_max(x1);
  y0 = wave_min(y0); y1 = wave_max(y1);
  __shared__ double part[4][4];
  if ((threadIdx.x & 63) == 0) {
    double* mine = part[threadIdx.x >> 6];
    mine[0] = x0; mine[1] = x1; mine[2] = y0; mine[3] = y1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      x0 = fmin(x0, part[w][0]); x1 = fmax(x1, part[w][1]);
      y0 = fmin(y0, part[w][2]); y1 = fmax(y1, part[w][3]);
    }
    if (x0 <= x1) {
      rs_lower(key + 0, rs_order_key(x0));
      rs_raise(key + 1, rs_order_key(x1));
      rs_lower(key + 2, rs_order_key(y0));
      rs_raise(key + 3, rs_order_key(y1));
    }
  }
}

// the pixel rule: t = (x - x0) * sx in two roundings, floor, the far edge and a rounded index >= W give W - 1
__device__ __forceinline__ int rs_index(double x, double x0, double x1, double sx, int W) {
#pragma clang fp contract(off)
  const double d = x - x0;
  const double t = d * sx;
  if (x == x1 || !(t < (double)W)) return W - 1;
  return (int)floor(t);
}

__global__ __launch_bounds__(256) void k_rs_pixel(const double* __restrict__ xy, int64_t n, double x0, double x1, double y0, double y1,
                                                  double sx, double sy, int W, int H, int32_t* __restrict__ pix,
                                                  int32_t* __restrict__ code, unsigned long long* __restrict__ ctr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool out = false;
  if (i < n) {
    const double x = xy[2 * i], y = xy[2 * i + 1];
    const bool fin = finite_d(x) && finite_d(y);
    const bool in = fin && x0 <= x && x <= x1 && y0 <= y && y <= y1;
    int32_t p = -1;
    if (in) p = rs_index(y, y0, y1, sy, H) * W + rs_index(x, x0, x1, sx, W);
    pix[i] = p;
    code[i] = p < 0 ? -1 : (p & (RS_DIGIT - 1));
    out = fin && !in;
  }
  const unsigned long long b = __ballot(out);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(ctr + RS_C_OUTSIDE, (unsigned long long)__popcll(b));
}

// ------------------------------------------------------------------ the sort's glue
// cnt[b][g] (B blocks x G digits) -> the count in the blocks before b; total[g]: what launch_block_scan computes, with the
// loads of 16 blocks in flight before their stores (one thread per digit otherwise waits for memory once per block)
__global__ __launch_bounds__(256) void k_rs_scan(unsigned int* __restrict__ cnt, int G, int B, int64_t* __restrict__ total) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  int64_t run = 0;
  for (int b0 = 0; b0 < B; b0 += 16) {
    unsigned int t[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) t[k] = b0 + k < B ? cnt[(int64_t)(b0 + k) * G + g] : 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (b0 + k < B) {
        cnt[(int64_t)(b0 + k) * G + g] = (unsigned int)run;
        run += t[k];
      }
  }
  total[g] = run;
}

// digit totals -> offsets, bptr[n_bins] = their sum; one workgroup
__global__ __launch_bounds__(256) void k_rs_bptr(const int64_t* __restrict__ tot, int n_bins, int64_t* __restrict__ bptr) {
  __shared__ int64_t part[256];
  const int t = threadIdx.x, per = (n_bins + 255) / 256;
  int64_t s = 0;
  for (int k = 0; k < per; ++k)
    if (t * per + k < n_bins) s += tot[t * per + k];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int64_t run = 0;
    for (int i = 0; i < 256; ++i) {
      const int64_t x = part[i];
      part[i] = run;
      run += x;
    }
    bptr[n_bins] = run;
  }
  __syncthreads();
  int64_t run = part[t];
  for (int k = 0; k < per; ++k)
    if (t * per + k < n_bins) {
      bptr[t * per + k] = run;
      run += tot[t * per + k];
    }
}

// pass 2 sorts position j of pass 1's list (m = *m_ptr of them) by the pixel's high bits
__global__ __launch_bounds__(256) void k_rs_code2(const int32_t* __restrict__ pix, const int32_t* __restrict__ perm1,
                                                  const int64_t* __restrict__ m_ptr, int64_t n, int32_t* __restrict__ code) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  code[j] = j < *m_ptr ? (pix[perm1[j]] >> RS_DIGIT_BITS) : -1;
}

// pstart / pend (zeroed before) of every pixel that has a cell
__global__ __launch_bounds__(256) void k_rs_bounds(const int32_t* __restrict__ pix, const int32_t* __restrict__ perm,
                                                   const int64_t* __restrict__ m_ptr, int32_t* __restrict__ pstart,
                                                   int32_t* __restrict__ pend) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, m = *m_ptr;
  if (j >= m) return;
  const int32_t p = pix[perm[j]];
  if (j == 0 || pix[perm[j - 1]] != p) pstart[p] = (int32_t)j;
  if (j == m - 1 || pix[perm[j + 1]] != p) pend[p] = (int32_t)(j + 1);
}

// n per pixel; the big pixels and their chunks.  Where a big pixel's records land depends on the scheduling, what is
// computed from them does not.  (At most n / (RS_SMALL + 1) big pixels and that plus n / RS_CHUNK chunks: the buffers' sizes.)
__global__ __launch_bounds__(256) void k_rs_classify(const int32_t* __restrict__ pstart, const int32_t* __restrict__ pend, int P,
                                                     int32_t* __restrict__ n_img, unsigned long long* __restrict__ ctr,
                                                     int32_t* __restrict__ slot, int32_t* __restrict__ big) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int cnt = pend[p] - pstart[p];
  n_img[p] = cnt;
  if (cnt > RS_SMALL) {
    const int nch = (cnt + RS_CHUNK - 1) / RS_CHUNK;
    const int64_t base = (int64_t)atomicAdd(ctr + RS_C_SLOTS, (unsigned long long)nch);
    const int64_t b = (int64_t)atomicAdd(ctr + RS_C_BIG, 1ull);
    big[3 * b] = p;
    big[3 * b + 1] = (int32_t)base;
    big[3 * b + 2] = nch;
    for (int k = 0; k < nch; ++k) {
      slot[2 * (base + k)] = p;
      slot[2 * (base + k) + 1] = k;
    }
  }
}

// ------------------------------------------------------------------ the reduction, per key (blockIdx.y)
struct RsKeys {
  const double* v;      // q x n
  const double* fdr;    // q x n (rows of keys without an fdr are not read)
  int64_t n;
  unsigned int has_fdr; // bit k: key k has an fdr
  double thresh;
  __device__ __forceinline__ bool pass(int k, int32_t cell, double* x) const {
    *x = v[(int64_t)k * n + cell];
    if (!finite_d(*x)) return false;
    return !((has_fdr >> k) & 1u) || fdr[(int64_t)k * n + cell] <= thresh;     // a NaN fdr fails
  }
};

struct RsImages {
  int32_t* n_pass;
  double *sum, *top, *bot;
  unsigned long long* absmax;     // per key: 0 = nothing passes, else 1 + the bits of the largest |v| (monotone for |v| >= 0)
};

__device__ __forceinline__ void rs_write(const RsImages& o, int k, int64_t at, bool on, double s, double mx, double mn, int np) {
  if (on) {
    o.n_pass[at] = np;
    o.sum[at] = np ? s : 0.0;
    o.top[at] = np ? mx : NAN;
    o.bot[at] = np ? mn : NAN;
  }
  double a = (on && np) ? fmax(fabs(mx), fabs(mn)) : -1.0;
  a = wave_max(a);
  if ((threadIdx.x & 63) == 0 && a >= 0.0) rs_raise(o.absmax + k, (unsigned long long)__double_as_longlong(a) + 1ull);
}

__global__ __launch_bounds__(256) void k_rs_small(RsKeys in, const int32_t* __restrict__ perm, const int32_t* __restrict__ pstart,
                                                  const int32_t* __restrict__ pend, int P, RsImages o) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
  const int lo = p < P ? pstart[p] : 0, hi = p < P ? pend[p] : 0;
  const bool on = p < P && hi - lo <= RS_SMALL;
  double s = 0.0, mx = -INFINITY, mn = INFINITY;
  int np = 0;
  if (on)
    for (int j = lo; j < hi; ++j) {
      double x;
      if (in.pass(k, perm[j], &x)) {
        s += x;
        mx = fmax(mx, x);
        mn = fmin(mn, x);
        ++np;
      }
    }
  rs_write(o, k, (int64_t)k * P + p, on, s, mx, mn, np);
}

// part[(k * nslots + slot) * 4] = sum, max, min, count of the chunk's passing cells
__global__ __launch_bounds__(64) void k_rs_chunk(RsKeys in, const int32_t* __restrict__ perm, const int32_t* __restrict__ pstart,
                                                 const int32_t* __restrict__ pend, const int32_t* __restrict__ slot, int64_t nslots,
                                                 double* __restrict__ part) {
  const int64_t sl = blockIdx.x;
  const int k = blockIdx.y, p = slot[2 * sl];
  const int64_t lo = pstart[p] + (int64_t)slot[2 * sl + 1] * RS_CHUNK;
  const int64_t hi = lo + RS_CHUNK < pend[p] ? lo + RS_CHUNK : pend[p];
  double s = 0.0, mx = -INFINITY, mn = INFINITY;
  int np = 0;
  for (int64_t j = lo + threadIdx.x; j < hi; j += 64) {
    double x;
    if (in.pass(k, perm[j], &x)) {
      s += x;
      mx = fmax(mx, x);
      mn = fmin(mn, x);
      ++np;
    }
  }
  s = wave_sum(s);
  mx = wave_max(mx);
  mn = wave_min(mn);
  np = wave_sum_int(np);
  if (threadIdx.x == 0) {
    double* o = part + ((int64_t)k * nslots + sl) * 4;
    o[0] = s;
    o[1] = mx;
    o[2] = mn;
    o[3] = (double)np;
  }
}

__global__ __launch_bounds__(64) void k_rs_fold(const int32_t* __restrict__ big, const double* __restrict__ part, int64_t nslots, int P,
                                                RsImages o) {
  const int k = blockIdx.y;
  const int32_t* b = big + 3 * (int64_t)blockIdx.x;
  const int p = b[0], nch = b[2];
  const double* mine = part + ((int64_t)k * nslots + b[1]) * 4;
  double s = 0.0, mx = -INFINITY, mn = INFINITY;
  int np = 0;
  for (int ch = threadIdx.x; ch < nch; ch += 64) {
    s += mine[4 * ch];
    mx = fmax(mx, mine[4 * ch + 1]);
    mn = fmin(mn, mine[4 * ch + 2]);
    np += (int)mine[4 * ch + 3];
  }
  s = wave_sum(s);
  mx = wave_max(mx);
  mn = wave_min(mn);
  np = wave_sum_int(np);
  rs_write(o, k, (int64_t)k * P + p, threadIdx.x == 0, s, mx, mn, np);
}

// ------------------------------------------------------------------ radius: the marker's footprint
// top_r[p] = max of top over the disc around p, bottom_r = min of bottom; an empty pixel holds NaN, which fmax / fmin pass over
__global__ __launch_bounds__(256) void k_rs_dilate(const double* __restrict__ top, const double* __restrict__ bot, int W, int H, int r,
                                                   double* __restrict__ topr, double* __restrict__ botr) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x, P = W * H;
  if (p >= P) return;
  const int64_t at = (int64_t)blockIdx.y * P;
  const int ix = p % W, iy = p / W;
  double mx = -INFINITY, mn = INFINITY;
  for (int dy = -r; dy <= r; ++dy) {
    const int y = iy + dy;
    if (y < 0 || y >= H) continue;
    for (int dx = -r; dx <= r; ++dx) {
      const int x = ix + dx;
      if (x < 0 || x >= W || dx * dx + dy * dy > r * r) continue;
      mx = fmax(mx, top[at + (int64_t)y * W + x]);
      mn = fmin(mn, bot[at + (int64_t)y * W + x]);
    }
  }
  topr[at + p] = mx == -INFINITY ? NAN : mx;
  botr[at + p] = mn == INFINITY ? NAN : mn;
}

__global__ __launch_bounds__(256) void k_rs_cover(const int32_t* __restrict__ n_img, int W, int H, int r, uint8_t* __restrict__ cov) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= W * H) return;
  const int ix = p % W, iy = p / W;
  bool any = false;
  for (int dy = -r; dy <= r; ++dy) {
    const int y = iy + dy;
    if (y < 0 || y >= H) continue;
    for (int dx = -r; dx <= r; ++dx) {
      const int x = ix + dx;
      if (x < 0 || x >= W || dx * dx + dy * dy > r * r) continue;
      any = any || n_img[(int64_t)y * W + x] > 0;
    }
  }
  cov[p] = any ? 1 : 0;
}

// one pass of the counting sort on codes that are on the device already: `count` entries, codes in [-1, n_bins)
template <class Pol>
int rs_sort_pass(cna_ctx* c, hipStream_t st, RasterWork* w, const Pol& pol, int64_t count, int n_bins, int32_t* out) {
  const int64_t rpb = round_up64((count + SORT_MAX_BLOCKS - 1) / SORT_MAX_BLOCKS, 64);
  const int64_t B = (count + rpb - 1) / rpb;
  CNA_TRY(buf_need(c, st, w->cnt, 4 * B * n_bins));
  hipLaunchKernelGGL((k_sort_count<Pol>), dim3((unsigned)B), dim3(256), 0, st, pol, w->code.as<const int32_t>(), count, n_bins, rpb,
                     w->cnt.as<unsigned int>(), w->tot.as<unsigned long long>(),
                     (int*)(w->ctr.as<unsigned long long>() + 4 + RS_C_BAD));
  hipLaunchKernelGGL(k_rs_scan, dim3((unsigned)((n_bins + 255) / 256)), dim3(256), 0, st, w->cnt.as<unsigned int>(), n_bins, (int)B,
                     w->tot.as<int64_t>());
  hipLaunchKernelGGL(k_rs_bptr, dim3(1), dim3(256), 0, st, w->tot.as<const int64_t>(), n_bins, w->bptr.as<int64_t>());
  hipLaunchKernelGGL((k_sort_fill<Pol>), dim3((unsigned)B), dim3(64), 0, st, pol, w->code.as<const int32_t>(), count, n_bins, rpb,
                     w->cnt.as<const unsigned int>(), w->bptr.as<const int64_t>(), out);
  HIP_TRY(hipGetLastError());
  return 0;
}

// out[i] = the int32 stored at ((int32_t*)out)[count + i], i ascending: the write of i ends where the read of i ends or before
void rs_widen(int64_t* out, int64_t count) {
  const char* src = reinterpret_cast<const char*>(out) + 4 * count;
  for (int64_t i = 0; i < count; ++i) {
    int32_t v;
    std::memcpy(&v, src + 4 * i, 4);
    out[i] = v;
  }
}

bool rs_finite(double x) { return std::fabs(x) <= 1.79769313486231570815e308; }

}  // namespace

extern "C" int cna_coef_raster(cna_ctx* c, const double* xy, const double* V, const double* FDR, const int32_t* has_fdr, int q,
                               int64_t n_cells, double fdr_thresh, double* extent, int auto_extent, int width, int height,
                               int radius, int64_t* n_out, int64_t* n_outside_out, int64_t* n_pass_out, double* sum_out,
                               double* top_out, double* bottom_out, uint8_t* covered_out, double* absmax_out) {
  CHECK_CTX(c);
  if (!xy || !V || !has_fdr || !extent || !n_out || !n_outside_out || !n_pass_out || !sum_out || !top_out || !bottom_out ||
      !absmax_out)
    CNA_FAIL(CNA_EINVAL, "cna_coef_raster: null pointer");
  if (n_cells < 1 || n_cells >= (1ll << 31)) CNA_FAIL(CNA_EINVAL, "cna_coef_raster: cells must lie in [1, 2^31)");
  if (q < 1 || q > RS_MAX_KEYS) CNA_FAIL(CNA_EINVAL, "cna_coef_raster: 1 <= q <= 16");
  if (width < 1 || width > RS_MAX_SIDE || height < 1 || height > RS_MAX_SIDE)
    CNA_FAIL(CNA_EINVAL, "cna_coef_raster: width and height must lie in [1, 4096]");
  if ((int64_t)q * width * height > RS_MAX_PIXELS) CNA_FAIL(CNA_EINVAL, "cna_coef_raster: q * width * height must not exceed 2^22");
  if (radius < 0 || radius > RS_MAX_RADIUS) CNA_FAIL(CNA_EINVAL, "cna_coef_raster: 0 <= radius <= 16");
  unsigned int fdr_mask = 0;
  for (int k = 0; k < q; ++k)
    if (has_fdr[k]) fdr_mask |= 1u << k;
  if (fdr_mask && !FDR) CNA_FAIL(CNA_EINVAL, "cna_coef_raster: a key has an fdr and FDR is null");
  if (!auto_extent) {
    for (int i = 0; i < 4; ++i)
      if (!rs_finite(extent[i])) CNA_FAIL(CNA_EINVAL, "cna_coef_raster: the extent must be finite");
    if (!(extent[1] > extent[0] && extent[3] > extent[2])) CNA_FAIL(CNA_EINVAL, "cna_coef_raster: the extent must be increasing");
  }
  ExprState* es = nullptr;
  CNA_TRY(expr_get_state(c, &es));
  hipStream_t st = es->st;
  RasterWork* w = expr_work<RasterWork>(es, EXPR_RASTER);
  const int64_t n = n_cells;
  const int W = width, H = height, P = W * H;
  const int64_t QP = (int64_t)q * P;
  const int64_t max_big = n / (RS_SMALL + 1) + 1, max_slots = max_big + n / RS_CHUNK + 1;
  CNA_TRY(buf_need(c, st, w->xy, 16 * n));
  CNA_TRY(buf_need(c, st, w->v, 8 * n * q));
  if (fdr_mask) CNA_TRY(buf_need(c, st, w->fdr, 8 * n * q));
  CNA_TRY(buf_need(c, st, w->pix, 4 * n));
  CNA_TRY(buf_need(c, st, w->code, 4 * n));
  CNA_TRY(buf_need(c, st, w->tot, 8 * RS_DIGIT));
  CNA_TRY(buf_need(c, st, w->bptr, 8 * (RS_DIGIT + 1)));
  CNA_TRY(buf_need(c, st, w->perm1, 4 * n));
  CNA_TRY(buf_need(c, st, w->perm2, 4 * n));
  CNA_TRY(buf_need(c, st, w->range, 4 * 2 * (int64_t)P));
  CNA_TRY(buf_need(c, st, w->ctr, 8 * (4 + RS_COUNTERS + RS_MAX_KEYS)));
  CNA_TRY(buf_need(c, st, w->slot, 4 * 2 * max_slots));
  CNA_TRY(buf_need(c, st, w->big, 4 * 3 * max_big));
  CNA_TRY(buf_need(c, st, w->n_img, 4 * (int64_t)P));
  CNA_TRY(buf_need(c, st, w->np_img, 4 * QP));
  CNA_TRY(buf_need(c, st, w->sum, 8 * QP));
  CNA_TRY(buf_need(c, st, w->top, 8 * QP));
  CNA_TRY(buf_need(c, st, w->bot, 8 * QP));
  if (radius > 0) {
    CNA_TRY(buf_need(c, st, w->topr, 8 * QP));
    CNA_TRY(buf_need(c, st, w->botr, 8 * QP));
  }
  if (covered_out) CNA_TRY(buf_need(c, st, w->cov, P));

  std::optional<ProfScope> span;
  span.emplace(c, CNA_K_RASTER_UPLOAD, st);
  HIP_TRY(hipMemcpyAsync(w->xy.p, xy, (size_t)(16 * n), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w->v.p, V, (size_t)(8 * n * q), hipMemcpyHostToDevice, st));
  for (int k = 0; k < q; ++k)
    if ((fdr_mask >> k) & 1u)
      HIP_TRY(hipMemcpyAsync(w->fdr.as<double>() + (int64_t)k * n, FDR + (int64_t)k * n, (size_t)(8 * n), hipMemcpyHostToDevice, st));
  unsigned long long ctr_h[4 + RS_COUNTERS + RS_MAX_KEYS] = {~0ull, 0ull, ~0ull, 0ull};
  unsigned long long* ctr = w->ctr.as<unsigned long long>();
  HIP_TRY(hipMemcpyAsync(ctr, ctr_h, sizeof(ctr_h), hipMemcpyHostToDevice, st));
  span.reset();
  span.emplace(c, CNA_K_RASTER, st);
  const unsigned cell_blocks = (unsigned)((n + 255) / 256), pix_blocks = (unsigned)((P + 255) / 256);

  double ext[4] = {extent[0], extent[1], extent[2], extent[3]};
  if (auto_extent) {
    hipLaunchKernelGGL(k_rs_extent, dim3(std::min(cell_blocks, 1024u)), dim3(256), 0, st, w->xy.as<const double>(), n, ctr);
    unsigned long long key[4];
    CNA_TRY(fetch_results(st, "cna_coef_raster", {{key, ctr, sizeof(key)}}));
    if (key[0] == ~0ull) {                      // no cell with finite coordinates: the extent is NaN, nothing else is written
      for (int i = 0; i < 4; ++i) extent[i] = NAN;
      return 0;
    }
    for (int i = 0; i < 4; ++i) ext[i] = rs_key_value(key[i]);
    for (int a = 0; a < 4; a += 2)
      if (ext[a] == ext[a + 1]) {               // as np.histogram widens a range without width
        const double v = ext[a];
        ext[a] = v - 0.5;
        ext[a + 1] = v + 0.5;
      }
    if (!(ext[1] > ext[0] && ext[3] > ext[2]))
      CNA_FAIL(CNA_EINVAL, "cna_coef_raster: the automatic extent has no width at this magnitude; pass one");
  }
  const double sx = (double)W / (ext[1] - ext[0]), sy = (double)H / (ext[3] - ext[2]);

  int32_t* pix = w->pix.as<int32_t>();
  int32_t* pstart = w->range.as<int32_t>();
  int32_t* pend = pstart + P;
  hipLaunchKernelGGL(k_rs_pixel, dim3(cell_blocks), dim3(256), 0, st, w->xy.as<const double>(), n, ext[0], ext[1], ext[2], ext[3], sx, sy,
                     W, H, pix, w->code.as<int32_t>(), ctr + 4);
  CNA_TRY(rs_sort_pass(c, st, w, RsCells{}, n, std::min(P, RS_DIGIT), w->perm1.as<int32_t>()));
  const int hi_bins = ((P - 1) >> RS_DIGIT_BITS) + 1;
  hipLaunchKernelGGL(k_rs_code2, dim3(cell_blocks), dim3(256), 0, st, (const int32_t*)pix, w->perm1.as<const int32_t>(),
                     w->bptr.as<const int64_t>() + std::min(P, RS_DIGIT), n, w->code.as<int32_t>());
  CNA_TRY(rs_sort_pass(c, st, w, RsPerm{w->perm1.as<const int32_t>()}, n, hi_bins, w->perm2.as<int32_t>()));
  const int32_t* perm = w->perm2.as<const int32_t>();
  HIP_TRY(hipMemsetAsync(pstart, 0, (size_t)(4 * 2 * (int64_t)P), st));
  hipLaunchKernelGGL(k_rs_bounds, dim3(cell_blocks), dim3(256), 0, st, (const int32_t*)pix, perm, w->bptr.as<const int64_t>() + hi_bins,
                     pstart, pend);
  hipLaunchKernelGGL(k_rs_classify, dim3(pix_blocks), dim3(256), 0, st, (const int32_t*)pstart, (const int32_t*)pend, P,
                     w->n_img.as<int32_t>(), ctr + 4, w->slot.as<int32_t>(), w->big.as<int32_t>());
  unsigned long long cnt_h[RS_COUNTERS];
  CNA_TRY(fetch_results(st, "cna_coef_raster", {{cnt_h, ctr + 4, sizeof(cnt_h)}}));
  const int64_t nslots = (int64_t)cnt_h[RS_C_SLOTS], nbig = (int64_t)cnt_h[RS_C_BIG];

  const RsKeys keys{w->v.as<const double>(), w->fdr.as<const double>(), n, fdr_mask, fdr_thresh};
  const RsImages img{w->np_img.as<int32_t>(), w->sum.as<double>(), w->top.as<double>(), w->bot.as<double>(), ctr + 4 + RS_COUNTERS};
  hipLaunchKernelGGL(k_rs_small, dim3(pix_blocks, (unsigned)q), dim3(256), 0, st, keys, perm, (const int32_t*)pstart, (const int32_t*)pend,
                     P, img);
  if (nslots) {
    CNA_TRY(buf_need(c, st, w->part, 8 * 4 * nslots * q));
    hipLaunchKernelGGL(k_rs_chunk, dim3((unsigned)nslots, (unsigned)q), dim3(64), 0, st, keys, perm, (const int32_t*)pstart,
                       (const int32_t*)pend, w->slot.as<const int32_t>(), nslots, w->part.as<double>());
    hipLaunchKernelGGL(k_rs_fold, dim3((unsigned)nbig, (unsigned)q), dim3(64), 0, st, w->big.as<const int32_t>(),
                       w->part.as<const double>(), nslots, P, img);
  }
  const double* top = img.top;
  const double* bot = img.bot;
  if (radius > 0) {
    hipLaunchKernelGGL(k_rs_dilate, dim3(pix_blocks, (unsigned)q), dim3(256), 0, st, top, bot, W, H, radius, w->topr.as<double>(),
                       w->botr.as<double>());
    top = w->topr.as<const double>();
    bot = w->botr.as<const double>();
  }
  if (covered_out)
    hipLaunchKernelGGL(k_rs_cover, dim3(pix_blocks), dim3(256), 0, st, w->n_img.as<const int32_t>(), W, H, radius, w->cov.as<uint8_t>());

  span.reset();
  span.emplace(c, CNA_K_RASTER_FETCH, st);
  // the counts are int32 on the device: each lands in the upper half of its int64 output and is widened in place from the front
  int32_t* n_h = reinterpret_cast<int32_t*>(n_out) + P;
  int32_t* np_h = reinterpret_cast<int32_t*>(n_pass_out) + QP;
  unsigned long long abs_h[RS_MAX_KEYS];
  if (covered_out) HIP_TRY(hipMemcpyAsync(covered_out, w->cov.p, (size_t)P, hipMemcpyDeviceToHost, st));
  CNA_TRY(fetch_results(st, "cna_coef_raster",
                        {{n_h, w->n_img.p, 4 * (size_t)P},
                         {np_h, w->np_img.p, 4 * (size_t)QP},
                         {sum_out, w->sum.p, 8 * (size_t)QP},
                         {top_out, top, 8 * (size_t)QP},
                         {bottom_out, bot, 8 * (size_t)QP},
                         {abs_h, ctr + 4 + RS_COUNTERS, 8 * (size_t)q}}));
  span.reset();
  rs_widen(n_out, P);
  rs_widen(n_pass_out, QP);
  *n_outside_out = (int64_t)cnt_h[RS_C_OUTSIDE];
  for (int k = 0; k < q; ++k) {
    const unsigned long long b = abs_h[k] - 1ull;
    double a = NAN;
    if (abs_h[k]) std::memcpy(&a, &b, 8);
    absmax_out[k] = a;
  }
  for (int i = 0; i < 4; ++i) extent[i] = ext[i];
  return 0;
}

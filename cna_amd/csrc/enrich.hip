// cna_enrichment_extremes: the running-sum extremes of gene set enrichment analysis for every gene set under every
// column of [r | null_r] (cna.tl.gene_set_test: the step demo/demo.ipynb, section 1.5, names after the per-gene
// correlations -- "they could be further analyzed using techniques like gene set enrichment analysis" -- with the
// phenotype permutations of cna.tl.gene_test as the null instead of permuted genes).
//
// Nothing here reads or writes the state of c_api.hip or the resident expression matrix: R, the sets and the buffers are this
// entry's own (EnrichWork), the stream is the expression stream.
//
//   k_en_check      one wave per set: every member in [0, n_genes), strictly ascending inside the set; the host reads the
//                   verdict before R goes up or any sum is formed
//   k_en_positions  one workgroup per (column, EN_BLOCK target genes), EN_TARGETS targets per lane in registers; the column
//                   goes through LDS in tiles of EN_TILE genes, read as broadcasts; a lane counts, for each of its targets,
//                   the valid genes with a larger value and those with an equal value and a smaller index: the target's
//                   place in np.argsort(-r, kind='stable') over the valid genes.  An invalid gene is staged as -inf, which
//                   is larger than or equal to no finite value: it counts for nobody.  A tile wholly before (after) the
//                   workgroup's targets needs one compare per pair, >= (>); only the tiles that overlap the targets compare
//                   indices.  Integer counts: exact, whatever the order.  The column's number of valid genes comes out of
//                   the staging of workgroup 0
//   k_en_extremes   one workgroup per (column, set), the sets dealt to four launches by size (64, 256, 1024, 4096 slots; one
//                   wave for the first two): the members' positions and weights into LDS, a bitonic sort on the positions
//                   (distinct among the valid members, so the order of the weights is the order of the positions whatever
//                   the schedule), the running weight S_j as an in-place scan in a fixed order (a lane's run of slots, the
//                   lanes of a wave, the waves in turn), then up_j = S_j / N_R - m_j / (Gv - k) and dn_j = S_(j-1) / N_R -
//                   m_j / (Gv - k), N_R = S_k itself, folded by fmax / fmin
// No floating-point atomics anywhere: two runs on one input give the same bits.
#include "expr.h"
#include <cmath>
#include <cstring>

// hipcc contracts a*b+c into an fma by default.  The weight r*r (weight = 2) is specified as a product rounded on its own and
// THEN added to the running sum, so that the sums are the ones a host restatement forms term by term; contraction is off
// for the whole file.
#pragma clang fp contract(off)

namespace {

constexpr int EN_MAX_COLS = 4096;
constexpr int EN_MAX_SETS = 1 << 20;
constexpr int EN_MAX_SIZE = 4096;
constexpr int EN_TILE = 2048;            // genes of the column per LDS tile of k_en_positions (16 KB)
constexpr int EN_THREADS = 256;
constexpr int EN_TARGETS = 4;            // target genes per lane: one LDS read serves four compares
constexpr int EN_BLOCK = EN_THREADS * EN_TARGETS;
constexpr uint32_t EN_NO_POS = 0xffffffffu;      // an invalid gene (positions are below 2^31)
constexpr int EN_CLASSES = 4;
constexpr int EN_CAP[EN_CLASSES] = {64, 256, 1024, 4096};

// R; the positions; the sets [ptr | genes | ids by class]; the verdict; [up | down | size | valid]
struct EnrichWork : BufSet {
  Buf R{*this}, pos{*this}, sptr{*this}, sgenes{*this}, ids{*this}, flag{*this}, out{*this};
};

__global__ __launch_bounds__(64) void k_en_check(const int64_t* __restrict__ sptr, const int32_t* __restrict__ sgenes, int n_sets,
                                                 int64_t G, int* __restrict__ bad) {
  for (int64_t s = blockIdx.x; s < n_sets; s += gridDim.x) {
    const int64_t lo = sptr[s], hi = sptr[s + 1];
    for (int64_t e = lo + threadIdx.x; e < hi; e += 64) {
      const int32_t g = sgenes[e];
      if (g < 0 || g >= G || (e > lo && sgenes[e - 1] >= g)) atomicOr(bad, 1);
    }
  }
}

// grid (tiles of EN_BLOCK targets, columns).  pos[c * G + g] = the place of gene g among the valid genes of column c in
// descending order of value, ties in gene order; EN_NO_POS for an invalid gene.  valid[c] = the valid genes of the column.
__global__ __launch_bounds__(EN_THREADS) void k_en_positions(const double* __restrict__ R, int64_t G, uint32_t* __restrict__ pos,
                                                             int32_t* __restrict__ valid) {
  __shared__ double sv[EN_TILE];
  __shared__ unsigned int nv;
  const int64_t c = blockIdx.y;
  const double* col = R + c * G;
  const int64_t t0 = (int64_t)blockIdx.x * EN_BLOCK;
  const int64_t t1 = t0 + EN_BLOCK < G ? t0 + EN_BLOCK : G;
  double rg[EN_TARGETS];
  int64_t g[EN_TARGETS];
  uint32_t cnt[EN_TARGETS];
  bool ok[EN_TARGETS];
#pragma unroll
  for (int k = 0; k < EN_TARGETS; ++k) {
    g[k] = t0 + threadIdx.x + (int64_t)k * EN_THREADS;
    const double v = g[k] < G ? col[g[k]] : NAN;
    ok[k] = finite_d(v);
    rg[k] = ok[k] ? v : INFINITY;              // nothing is larger than or equal to it: the count is not used anyway
    cnt[k] = 0u;
  }
  if (threadIdx.x == 0) nv = 0u;
  unsigned int mine = 0u;
  for (int64_t base = 0; base < G; base += EN_TILE) {
    __syncthreads();
    for (int i = threadIdx.x; i < EN_TILE; i += EN_THREADS) {
      const int64_t h = base + i;
      const double v = h < G ? col[h] : NAN;
      const bool f = finite_d(v);
      mine += f ? 1u : 0u;
      sv[i] = f ? v : -INFINITY;
    }
    __syncthreads();
    const int len = (int)(G - base < EN_TILE ? G - base : EN_TILE);
    const int lim = (len + 3) & ~3;            // the slots past len hold -inf
    if (base + EN_TILE <= t0) {                // every gene of the tile before every target: a tie counts
      for (int i = 0; i < lim; ++i) {
        const double x = sv[i];
#pragma unroll
        for (int k = 0; k < EN_TARGETS; ++k) cnt[k] += x >= rg[k] ? 1u : 0u;
      }
    } else if (base >= t1) {                   // ... after every target: a tie does not
      for (int i = 0; i < lim; ++i) {
        const double x = sv[i];
#pragma unroll
        for (int k = 0; k < EN_TARGETS; ++k) cnt[k] += x > rg[k] ? 1u : 0u;
      }
    } else {
      for (int i = 0; i < lim; ++i) {
        const double x = sv[i];
        const int64_t h = base + i;
#pragma unroll
        for (int k = 0; k < EN_TARGETS; ++k) cnt[k] += (x > rg[k] || (x == rg[k] && h < g[k])) ? 1u : 0u;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < EN_TARGETS; ++k)
    if (g[k] < G) pos[c * G + g[k]] = ok[k] ? cnt[k] : EN_NO_POS;
  if (blockIdx.x == 0) {
    if (mine) atomicAdd(&nv, mine);
    __syncthreads();
    if (threadIdx.x == 0) valid[c] = (int32_t)nv;
  }
}

__device__ __forceinline__ double en_weight(double r, int weight) { return weight == 0 ? 1.0 : (weight == 1 ? fabs(r) : r * r); }

// grid (sets of this size class, columns); ids[blockIdx.x] = the set.  CAP slots, THREADS lanes (a power of two each).
template <int CAP, int THREADS>
__global__ __launch_bounds__(THREADS) void k_en_extremes(const double* __restrict__ R, const uint32_t* __restrict__ pos,
                                                         const int32_t* __restrict__ valid, int64_t G,
                                                         const int64_t* __restrict__ sptr, const int32_t* __restrict__ sgenes,
                                                         const int32_t* __restrict__ ids, int n_sets, int weight,
                                                         double* __restrict__ up, double* __restrict__ down,
                                                         int32_t* __restrict__ size) {
  constexpr int WAVES = THREADS / 64;
  __shared__ uint32_t key[CAP];
  __shared__ double sw[CAP];
  __shared__ double wtot[WAVES], rmax[WAVES], rmin[WAVES];
  __shared__ unsigned int nk;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = ids[blockIdx.x];
  const int64_t c = blockIdx.y;
  const int64_t lo = sptr[s];
  const int members = (int)(sptr[s + 1] - lo);
  int n = 2;
  while (n < members) n <<= 1;                 // <= CAP by the set's class
  if (tid == 0) nk = 0u;
  __syncthreads();
  unsigned int mine = 0u;
  for (int i = tid; i < n; i += THREADS) {
    uint32_t p = EN_NO_POS;
    double w = 0.0;
    if (i < members) {
      const int64_t at = c * G + sgenes[lo + i];
      p = pos[at];
      if (p != EN_NO_POS) {
        w = en_weight(R[at], weight);
        ++mine;
      }
    }
    key[i] = p;                                // the invalid members and the padding sort behind the valid ones, weight 0
    sw[i] = w;
  }
  if (mine) atomicAdd(&nk, mine);
  for (int span = 2; span <= n; span <<= 1) {
    for (int stride = span >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < (n >> 1); t += THREADS) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const bool asc = (i & span) == 0;
        const uint32_t a = key[i], b = key[j];
        if ((a > b) == asc) {
          key[i] = b;
          key[j] = a;
          const double x = sw[i];
          sw[i] = sw[j];
          sw[j] = x;
        }
      }
    }
  }
  __syncthreads();
  // S_j in place: a lane's run of slots in order, the lanes of a wave in order, the waves in order
  const int run = n >= THREADS ? n / THREADS : 1;
  const bool act = tid * run < n;
  double sum = 0.0;
  if (act)
    for (int i = tid * run; i < tid * run + run; ++i) {
      sum += sw[i];
      sw[i] = sum;
    }
  double inc = sum;
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  double before = __shfl_up(inc, 1, 64);
  if (lane == 0) before = 0.0;
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  double woff = 0.0;
  for (int w = 0; w < wave; ++w) woff += wtot[w];
  const double lead = woff + before;           // 0 for the first lane: its sums stay as they are
  if (act)
    for (int i = tid * run; i < tid * run + run; ++i) sw[i] = lead + sw[i];
  __syncthreads();
  const int k = (int)nk, Gv = valid[c];
  // N_R is S_k itself, not the scan's last slot (the same terms and zeros, but added in another order): S_k / N_R is
  // exactly 1 and up >= 0 holds to the bit
  const double NR = k ? sw[k - 1] : 0.0;
  const int64_t o = c * n_sets + s;
  if (k == 0 || k == Gv || NR == 0.0) {
    if (tid == 0) {
      up[o] = NAN;
      down[o] = NAN;
      size[o] = k;
    }
    return;
  }
  const double misses = (double)(Gv - k);
  double mx = -INFINITY, mn = INFINITY;
  for (int i = tid; i < k; i += THREADS) {
    const double miss = (double)(key[i] - (uint32_t)i) / misses;      // the misses before hit i
    const double hit = sw[i] / NR, prev = (i ? sw[i - 1] : 0.0) / NR;
    mx = fmax(mx, hit - miss);
    mn = fmin(mn, prev - miss);
  }
  mx = wave_max(mx);
  mn = wave_min(mn);
  if (lane == 0) {
    rmax[wave] = mx;
    rmin[wave] = mn;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < WAVES; ++w) {
      mx = fmax(mx, rmax[w]);
      mn = fmin(mn, rmin[w]);
    }
    up[o] = mx;
    down[o] = mn;
    size[o] = k;
  }
}

template <int CAP, int THREADS>
void launch_extremes(hipStream_t st, int count, int n_cols, const double* R, const uint32_t* pos, const int32_t* valid, int64_t G,
                     const int64_t* sptr, const int32_t* sgenes, const int32_t* ids, int n_sets, int weight, double* up,
                     double* down, int32_t* size) {
  if (count)
    hipLaunchKernelGGL((k_en_extremes<CAP, THREADS>), dim3((unsigned)count, (unsigned)n_cols), dim3(THREADS), 0, st, R, pos, valid,
                       G, sptr, sgenes, ids, n_sets, weight, up, down, size);
}

}  // namespace

extern "C" int cna_enrichment_extremes(cna_ctx* c, const double* R, int64_t n_cols, int64_t n_genes, const int64_t* set_ptr,
                                       const int32_t* set_genes, int n_sets, int weight, double* up_out, double* down_out,
                                       int32_t* size_out, int32_t* valid_out) {
  CHECK_CTX(c);
  if (!R || !set_ptr || !set_genes || !up_out || !down_out || !size_out || !valid_out)
    CNA_FAIL(CNA_EINVAL, "cna_enrichment_extremes: null pointer");
  if (n_cols < 1 || n_cols > EN_MAX_COLS) CNA_FAIL(CNA_EINVAL, "cna_enrichment_extremes: 1 <= n_cols <= 4096");
  if (n_genes < 1 || n_genes >= (1ll << 31)) CNA_FAIL(CNA_EINVAL, "cna_enrichment_extremes: genes must lie in [1, 2^31)");
  if (n_sets < 1 || n_sets > EN_MAX_SETS) CNA_FAIL(CNA_EINVAL, "cna_enrichment_extremes: 1 <= n_sets <= 2^20");
  if (weight < 0 || weight > 2)
    CNA_FAIL(CNA_EINVAL, "cna_enrichment_extremes: weight is 0, 1 or 2 (|r|^weight as 1, fabs(r), r * r; pow rounds differently "
                         "on the host and on the device)");
  if (set_ptr[0] != 0) CNA_FAIL(CNA_EINVAL, "cna_enrichment_extremes: set_ptr must start at 0");
  // the sets by size class: ids = [class 0 | class 1 | ...], the sets of a class ascending
  int64_t cls_n[EN_CLASSES] = {0, 0, 0, 0};
  std::vector<int8_t> cls((size_t)n_sets);
  for (int s = 0; s < n_sets; ++s) {
    const int64_t m = set_ptr[s + 1] - set_ptr[s];
    if (m < 0) CNA_FAIL(CNA_EINVAL, "cna_enrichment_extremes: set_ptr must not fall");
    if (m > EN_MAX_SIZE) CNA_FAIL(CNA_EINVAL, "cna_enrichment_extremes: a set has more than 4096 members");
    if (set_ptr[s + 1] >= (1ll << 31)) CNA_FAIL(CNA_EINVAL, "cna_enrichment_extremes: total membership must lie below 2^31");
    int k = 0;
    while (m > EN_CAP[k]) ++k;
    cls[(size_t)s] = (int8_t)k;
    ++cls_n[k];
  }
  const int64_t total = set_ptr[n_sets];
  int64_t cls_lo[EN_CLASSES + 1] = {0};
  for (int k = 0; k < EN_CLASSES; ++k) cls_lo[k + 1] = cls_lo[k] + cls_n[k];
  std::vector<int32_t> ids((size_t)n_sets);
  {
    int64_t cur[EN_CLASSES];
    for (int k = 0; k < EN_CLASSES; ++k) cur[k] = cls_lo[k];
    for (int s = 0; s < n_sets; ++s) ids[(size_t)cur[cls[(size_t)s]]++] = s;
  }
  ExprState* es = nullptr;
  CNA_TRY(expr_get_state(c, &es));
  hipStream_t st = es->st;
  EnrichWork* w = expr_work<EnrichWork>(es, EXPR_ENRICH);
  const int64_t G = n_genes, cells = n_cols * G, pairs = n_cols * (int64_t)n_sets;
  CNA_TRY(buf_need(c, st, w->sptr, 8 * ((int64_t)n_sets + 1)));
  CNA_TRY(buf_need(c, st, w->sgenes, 4 * std::max<int64_t>(1, total)));
  CNA_TRY(buf_need(c, st, w->ids, 4 * (int64_t)n_sets));
  CNA_TRY(buf_need(c, st, w->flag, 256));
  HIP_TRY(hipMemcpyAsync(w->sptr.p, set_ptr, (size_t)(8 * ((int64_t)n_sets + 1)), hipMemcpyHostToDevice, st));
  if (total) HIP_TRY(hipMemcpyAsync(w->sgenes.p, set_genes, (size_t)(4 * total), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w->ids.p, ids.data(), (size_t)(4 * (int64_t)n_sets), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(w->flag.p, 0, 4, st));
  const int64_t* sptr = w->sptr.as<const int64_t>();
  const int32_t* sgenes = w->sgenes.as<const int32_t>();
  // the members are judged before R goes up and before any sum is formed
  hipLaunchKernelGGL(k_en_check, dim3((unsigned)std::min(n_sets, 4096)), dim3(64), 0, st, sptr, sgenes, n_sets, G, w->flag.as<int>());
  HIP_TRY(hipGetLastError());
  int bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, w->flag.p, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (bad)
    CNA_FAIL(CNA_EINVAL, "cna_enrichment_extremes: a set member lies outside [0, n_genes) or the members of a set do not ascend strictly");
  // [up | down | size | valid]
  const int64_t out_bytes = 8 * pairs * 2 + 4 * pairs + 4 * n_cols;
  CNA_TRY(buf_need(c, st, w->R, 8 * cells));
  CNA_TRY(buf_need(c, st, w->pos, 4 * cells));
  CNA_TRY(buf_need(c, st, w->out, out_bytes));
  HIP_TRY(hipMemcpyAsync(w->R.p, R, (size_t)(8 * cells), hipMemcpyHostToDevice, st));
  const double* Rd = w->R.as<const double>();
  double* up = w->out.as<double>();
  double* down = up + pairs;
  int32_t* size = reinterpret_cast<int32_t*>(down + pairs);
  int32_t* valid = size + pairs;
  {
    ProfScope ps(c, CNA_K_ENRICH_POSITIONS, st);
    hipLaunchKernelGGL(k_en_positions, dim3((unsigned)((G + EN_BLOCK - 1) / EN_BLOCK), (unsigned)n_cols), dim3(EN_THREADS), 0, st, Rd,
                       G, w->pos.as<uint32_t>(), valid);
  }
  {
    ProfScope ps(c, CNA_K_ENRICH_EXTREMES, st);
    const uint32_t* pos = w->pos.as<const uint32_t>();
    const int32_t* idd = w->ids.as<const int32_t>();
    const int nc = (int)n_cols;
    launch_extremes<64, 64>(st, (int)cls_n[0], nc, Rd, pos, valid, G, sptr, sgenes, idd + cls_lo[0], n_sets, weight, up, down, size);
    launch_extremes<256, 64>(st, (int)cls_n[1], nc, Rd, pos, valid, G, sptr, sgenes, idd + cls_lo[1], n_sets, weight, up, down, size);
    launch_extremes<1024, 256>(st, (int)cls_n[2], nc, Rd, pos, valid, G, sptr, sgenes, idd + cls_lo[2], n_sets, weight, up, down, size);
    launch_extremes<4096, 256>(st, (int)cls_n[3], nc, Rd, pos, valid, G, sptr, sgenes, idd + cls_lo[3], n_sets, weight, up, down, size);
  }
  // the caller's buffers are written only once everything has succeeded
  std::vector<char> host((size_t)out_bytes);
  CNA_TRY(fetch_results(st, "cna_enrichment_extremes", {{host.data(), w->out.p, (size_t)out_bytes}}));
  const char* h = host.data();
  std::memcpy(up_out, h, 8 * (size_t)pairs);
  std::memcpy(down_out, h + 8 * pairs, 8 * (size_t)pairs);
  std::memcpy(size_out, h + 16 * pairs, 4 * (size_t)pairs);
  std::memcpy(valid_out, h + 20 * pairs, 4 * (size_t)n_cols);
  return 0;
}

// Connected components of the resident graph inside classes of cells (cna.tl.coef_populations): which connected groups of
// same-sign, FDR-passing neighbourhoods an association finds, how big each is and which cells it holds.  Every cell has a
// class (>= 0) or none (-1); two classed cells belong to one component when a chain of stored entries joins them, read in
// either direction, every cell on the chain being of their class (weak connectivity: an asymmetric graph is fine; self
// loops and duplicates change nothing).  An entry is an edge whatever its value -- a stored zero included: the graph is
// resident with every stored entry, and c->data is never read here.
//
// Nothing here writes the state of c_api.hip: the graph (c->indptr, c->indices, c->orig_idx) is read where it is, in the
// device's cell order, the buffers are this file's own (ComponentsWork), the stream is the expression stream, which waits
// for whatever the main stream has queued (a renumbering of the graph among it).
//
// The 8 XCDs' L2s are not coherent for plain stores inside a launch, so inside a launch parent[] is written ONLY by
// agent-scope atomics and every read of it that decides anything is an agent-scope atomic load or what an atomic
// returned; everything else is handed from kernel to kernel.
//
//   parent[x] <= x always; x is a root when parent[x] == x; a tree's root is its smallest cell.
//   cc_find     follows parent[] down (the value strictly decreases: bounded) and shortens the path it walks by
//               atomicMin(&parent[x], grandparent).  A value that was ever in parent[y] is a cell of y's tree for good (trees
//               only merge), and it is smaller than y, so it cannot lie below y: hanging y under it keeps the tree a tree.
//               A stale read costs chasing, never the result.
//   cc_unite    finds both roots; equal: done; else atomicCAS(&parent[hi], hi, lo) -- it succeeds only on a cell that IS
//               a root at that moment, so no link is ever overwritten (atomicMin on a non-root would lose its old link);
//               if it fails, it returned hi's parent, and the pair (that parent, lo) is taken up: the larger of the two
//               strictly decreases from try to try.  No thread waits for another; there is no lock and no flag.
//   k_cc_rows   16 lanes per row, a row without a class left at once; a row of more than CC_HUB entries goes onto a list.
//               An entry whose other end already points at the row's root costs three reads and no atomic.  The first
//               round hooks entry 0 of every row, flattens, entry 1, flattens, and only then the rest: on a kNN graph
//               the trees are then nearly final and flat, and the bulk of the entries takes that short way (hooking
//               everything at once built deep trees under contention: 11 ms at 2M cells x 30 in one class)
//   k_cc_hubs   ... and is spread over a whole grid, entry by entry
//   k_cc_flatten  parent[x] = root of x, for every classed cell (no hooking runs beside it: a cell seen as a root is one)
//   check       the same two kernels counting the same-class entries whose ends have different roots.  The host reads that
//               one count; not zero: hook, flatten and check again from the current state, CC_MAX_ROUNDS at most
//   k_cc_tally  size and smallest caller index per root: integer atomics, one per wave and root (exact, order-free)
//   k_cc_compact  the roots with at least min_cells cells -> a list {class, size, smallest caller index} (its order is
//               that of arrival: the caller sorts it), slot[root] = place in the list; components per class before the filter
//   k_cc_label  comp[caller index of x] = rank[slot[root of x]], -1 without a class or with a filtered component
// No floating point anywhere: two runs give the same arrays once the list is sorted.
#include "expr.h"
#include <climits>
#include <cstring>
#include <optional>

namespace {

constexpr int CC_SUB = 16;                  // lanes per row: the typical row has 30-60 entries
constexpr int64_t CC_HUB = 1024;            // a row with more entries is walked by CC_HUB_BLOCKS workgroups
constexpr int CC_HUB_BLOCKS = 256;
constexpr int CC_MAX_ROUNDS = 32;
constexpr int CC_SAMPLES = 2;               // launches over ONE entry of every row, each flattened, before the launch over the rest
constexpr int64_t CC_ALL = INT64_MAX;
constexpr int CC_MAX_CLASSES = 1 << 24;
constexpr unsigned CC_MAX_GRID = 1u << 18;

enum { CC_C_HUBS = 0, CC_C_BAD_EDGES, CC_C_KEPT, CC_C_BAD_CODE, CC_COUNTERS };   // unsigned long long each

struct ComponentsWork : BufSet {
  Buf codes{*this};                                   // the classes in the caller's order, as uploaded
  Buf cls{*this}, parent{*this}, size{*this}, first{*this}, slot{*this};   // int32 per cell, device order
  Buf hubs{*this}, ctr{*this}, totals{*this};
  Buf list{*this};                                    // [class | size | first], n each
  Buf rank{*this}, comp{*this};
  // what the last cna_graph_components_find left for _list and _label: valid while the graph it read is the resident one
  int64_t n = 0, kept = -1;
  const void* indptr = nullptr;
  const void* orig = nullptr;
};

#define CC_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ int cc_load(const int32_t* p) { return __hip_atomic_load(p, CC_RLX); }

__device__ __forceinline__ int cc_find(int32_t* parent, int x) {
  int p = cc_load(parent + x);
  while (p < x) {                                     // x strictly decreases
    const int gp = cc_load(parent + p);
    if (gp < p) (void)__hip_atomic_fetch_min(parent + x, gp, CC_RLX);
    x = p;
    p = gp;
  }
  return x;
}

// joins the trees of a and b; returns a cell of the joined tree that is no larger than either root it saw
__device__ __forceinline__ int cc_unite(int32_t* parent, int a, int b) {
  for (;;) {                                          // max(a, b) after the finds strictly decreases
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return a;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    int expected = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, CC_RLX)) return lo;
    if (expected >= hi) return lo;                    // (cannot happen: parent[hi] <= hi, and it was not hi)
    a = expected;
    b = lo;
  }
}

__device__ __forceinline__ unsigned long long cc_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int cc_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}

// cls[i] = the class of the caller's cell orig[i] (a code outside [-1, n_classes) is flagged and dropped), parent[i] = i
__global__ __launch_bounds__(256) void k_cc_init(const int32_t* __restrict__ codes, const int64_t* __restrict__ orig, int64_t n,
                                                 int n_classes, int32_t* __restrict__ cls, int32_t* __restrict__ parent,
                                                 int32_t* __restrict__ size, int32_t* __restrict__ first,
                                                 int32_t* __restrict__ slot, unsigned long long* __restrict__ ctr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t o = orig ? orig[i] : i;
  int c = -1;
  if (o >= 0 && o < n) c = codes[o];
  if (c < -1 || c >= n_classes) {
    atomicOr(ctr + CC_C_BAD_CODE, 1ull);
    c = -1;
  }
  cls[i] = c;
  parent[i] = (int32_t)i;
  size[i] = 0;
  first[i] = INT_MAX;
  slot[i] = -1;
}

// one entry of row `row` (class cu): hook (cur: a cell of row's tree, kept near its root) or check (ru: row's root)
template <bool CHECK>
__device__ __forceinline__ void cc_entry(const int32_t* __restrict__ cls, int32_t* parent, int64_t n, int row, int cu, int v,
                                         int ru, int& cur, unsigned long long& bad) {
  if ((unsigned)v >= (unsigned)n || v == row) return;
  if (cls[v] != cu) return;
  if (CHECK) {
    bad += parent[v] != ru ? 1ull : 0ull;
  } else {
    const int pv = cc_load(parent + v);               // a cell of v's tree: equal to a cell of row's tree, the trees are one
    if (pv != cur) cur = cc_unite(parent, cur, pv);
  }
}

template <bool CHECK>
__global__ __launch_bounds__(256) void k_cc_rows(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                 const int32_t* __restrict__ cls, int32_t* parent, int64_t n, int64_t nnz,
                                                 int64_t e_lo, int64_t e_hi, int32_t* __restrict__ hubs, int64_t hub_cap,
                                                 unsigned long long* ctr) {
  const int sub = threadIdx.x & (CC_SUB - 1);
  const int64_t groups = (int64_t)gridDim.x * (256 / CC_SUB);
  unsigned long long bad = 0;
  for (int64_t row = (int64_t)blockIdx.x * (256 / CC_SUB) + (threadIdx.x / CC_SUB); row < n; row += groups) {
    const int cu = cls[row];
    if (cu < 0) continue;
    int64_t s0 = indptr[row], s1 = indptr[row + 1];
    if (s0 < 0) s0 = 0;
    if (s1 > nnz) s1 = nnz;
    if (e_hi - e_lo > CC_HUB && s1 - s0 > CC_HUB) {   // (a launch over a few entries of every row takes the hubs' too)
      if (!CHECK && sub == 0) {
        const unsigned long long at = atomicAdd(ctr + CC_C_HUBS, 1ull);
        if ((int64_t)at < hub_cap) hubs[at] = (int32_t)row;
      }
      continue;
    }
    if (s1 - s0 > e_hi) s1 = s0 + e_hi;
    s0 += e_lo;
    if (s0 >= s1) continue;
    int cur = CHECK ? 0 : cc_find(parent, (int)row);
    const int ru = CHECK ? parent[row] : 0;
    for (int64_t e = s0 + sub; e < s1; e += CC_SUB) cc_entry<CHECK>(cls, parent, n, (int)row, cu, idx[e], ru, cur, bad);
  }
  if (CHECK) {
    bad = cc_wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(ctr + CC_C_BAD_EDGES, bad);
  }
}

// the rows on the hub list (written by k_cc_rows<false> of this round), each spread over the whole grid
template <bool CHECK>
__global__ __launch_bounds__(256) void k_cc_hubs(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                 const int32_t* __restrict__ cls, int32_t* parent, int64_t n, int64_t nnz,
                                                 const int32_t* __restrict__ hubs, int64_t hub_cap,
                                                 unsigned long long* ctr) {
  int64_t nh = (int64_t)ctr[CC_C_HUBS];
  if (nh > hub_cap) nh = hub_cap;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long bad = 0;
  for (int64_t h = 0; h < nh; ++h) {
    const int row = hubs[h];
    if ((unsigned)row >= (unsigned)n) continue;
    const int cu = cls[row];
    int64_t s0 = indptr[row], s1 = indptr[row + 1];
    if (s0 < 0) s0 = 0;
    if (s1 > nnz) s1 = nnz;
    int cur = CHECK ? 0 : cc_find(parent, row);
    const int ru = CHECK ? parent[row] : 0;
    for (int64_t e = s0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < s1; e += stride)
      cc_entry<CHECK>(cls, parent, n, row, cu, idx[e], ru, cur, bad);
  }
  if (CHECK) {
    bad = cc_wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(ctr + CC_C_BAD_EDGES, bad);
  }
}

__global__ __launch_bounds__(256) void k_cc_flatten(const int32_t* __restrict__ cls, int32_t* parent, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || cls[i] < 0) return;
  const int r = cc_find(parent, (int)i);
  (void)__hip_atomic_fetch_min(parent + i, r, CC_RLX);
}

// size[root] += cells, first[root] = min caller index: the lanes of a wave that share a root send one atomic of each
__global__ __launch_bounds__(256) void k_cc_tally(const int32_t* __restrict__ cls, const int32_t* __restrict__ parent,
                                                  const int64_t* __restrict__ orig, int64_t n, int32_t* size, int32_t* first) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool active = i < n && cls[i] >= 0;
  const int r = active ? parent[i] : -1;
  const int o = active ? (int)(orig ? orig[i] : i) : INT_MAX;
  unsigned long long todo = __ballot(active);
  while (todo) {                                      // one turn per distinct root among the wave's cells
    const int leader = __ffsll((long long)todo) - 1;
    const int r0 = __shfl(r, leader, 64);
    const bool mine = active && r == r0;
    const unsigned long long m = __ballot(mine);
    const int mn = cc_wave_min(mine ? o : INT_MAX);
    if (lane == leader) {
      atomicAdd(size + r0, (int)__popcll(m));
      atomicMin(first + r0, mn);
    }
    todo &= ~m;
  }
}

// the roots: totals[class] += 1; those with size >= min_cells into the list, slot[root] = their place in it
__global__ __launch_bounds__(256) void k_cc_compact(const int32_t* __restrict__ cls, const int32_t* __restrict__ parent,
                                                    const int32_t* __restrict__ size, const int32_t* __restrict__ first, int64_t n,
                                                    int64_t min_cells, unsigned long long* totals, unsigned long long* ctr,
                                                    int32_t* __restrict__ lcls, int32_t* __restrict__ lsize,
                                                    int32_t* __restrict__ lfirst, int32_t* __restrict__ slot) {
  __shared__ unsigned int wcount[4];
  __shared__ unsigned long long base;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = i < n ? cls[i] : -1;
  const bool root = c >= 0 && parent[i] == (int32_t)i;
  unsigned long long todo = __ballot(root);
  while (todo) {                                      // one turn per distinct class among the wave's roots
    const int leader = __ffsll((long long)todo) - 1;
    const int c0 = __shfl(c, leader, 64);
    const unsigned long long m = __ballot(root && c == c0);
    if (lane == leader) atomicAdd(totals + c0, (unsigned long long)__popcll(m));
    todo &= ~m;
  }
  const bool kept = root && (int64_t)size[i] >= min_cells;
  const unsigned long long km = __ballot(kept);
  if (lane == 0) wcount[wave] = (unsigned int)__popcll(km);
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int t = wcount[0] + wcount[1] + wcount[2] + wcount[3];
    base = t ? atomicAdd(ctr + CC_C_KEPT, (unsigned long long)t) : 0ull;
  }
  __syncthreads();
  if (kept) {
    unsigned long long j = base + (unsigned long long)__popcll(km & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) j += wcount[w];
    if (j < (unsigned long long)n) {                  // (at most n roots: always)
      lcls[j] = c;
      lsize[j] = size[i];
      lfirst[j] = first[i];
      slot[i] = (int32_t)j;
    }
  }
}

__global__ __launch_bounds__(256) void k_cc_label(const int32_t* __restrict__ cls, const int32_t* __restrict__ parent,
                                                  const int32_t* __restrict__ slot, const int32_t* __restrict__ rank,
                                                  int64_t kept, const int64_t* __restrict__ orig, int64_t n,
                                                  int32_t* __restrict__ comp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t o = orig ? orig[i] : i;
  if (o < 0 || o >= n) return;
  int j = -1;
  if (cls[i] >= 0) {
    const int r = parent[i];
    if ((unsigned)r < (unsigned)n) j = slot[r];
  }
  if (j >= 0 && (int64_t)j < kept) comp[o] = rank ? rank[j] : j;
  else comp[o] = -1;
}

// the resident graph as this file can read it: one rank holding every row, cells and entries within int32
int cc_graph(cna_ctx* c, const char* who) {
  if (!c->indptr) CNA_FAIL(CNA_ESTATE, std::string(who) + " before cna_graph_upload");
  if (comm_active(c) || c->nranks != 1 || c->local_view || c->n_local != c->n_global)
    CNA_FAIL(CNA_ESTATE, std::string(who) + ": one rank holding the whole graph only (a cross-rank union is not built)");
  if (c->n_global < 1 || c->n_global >= (1ll << 31)) CNA_FAIL(CNA_EINVAL, std::string(who) + ": cells must lie in [1, 2^31)");
  return 0;
}

int cc_work(cna_ctx* c, const char* who, int64_t n_cells, int64_t n_kept, ExprState** es, ComponentsWork** w) {
  CNA_TRY(cc_graph(c, who));
  CNA_TRY(expr_get_state(c, es));
  *w = expr_work<ComponentsWork>(*es, EXPR_COMPONENTS);
  if ((*w)->kept < 0 || (*w)->indptr != c->indptr || (*w)->orig != c->orig_idx || (*w)->n != c->n_global)
    CNA_FAIL(CNA_ESTATE, std::string(who) + " needs cna_graph_components_find on the resident graph first");
  if (n_cells >= 0 && n_cells != (*w)->n) CNA_FAIL(CNA_EINVAL, std::string(who) + ": n_cells is not what the find saw");
  if (n_kept != (*w)->kept) CNA_FAIL(CNA_EINVAL, std::string(who) + ": n_kept is not what the find returned");
  return 0;
}

}  // namespace

extern "C" int cna_graph_components_find(cna_ctx* c, const int32_t* codes, int64_t n_cells, int n_classes, int64_t min_cells,
                                         int64_t* n_kept_out, int64_t* totals_out, int* sweeps_out) {
  CHECK_CTX(c);
  if (!codes || !n_kept_out || !totals_out || !sweeps_out) CNA_FAIL(CNA_EINVAL, "cna_graph_components_find: null pointer");
  CNA_TRY(cc_graph(c, "cna_graph_components_find"));
  if (n_cells != c->n_global)
    CNA_FAIL(CNA_EINVAL, "cna_graph_components_find: " + std::to_string(n_cells) + " codes, the graph has " +
                             std::to_string(c->n_global) + " cells");
  if (n_classes < 1 || n_classes > CC_MAX_CLASSES) CNA_FAIL(CNA_EINVAL, "cna_graph_components_find: 1 <= n_classes <= 2^24");
  ExprState* es = nullptr;
  CNA_TRY(expr_get_state(c, &es));
  hipStream_t st = es->st;
  ComponentsWork* w = expr_work<ComponentsWork>(es, EXPR_COMPONENTS);
  w->kept = -1;
  const int64_t n = n_cells, nnz = c->nnz, hub_cap = nnz / CC_HUB + 1;
  for (Buf* b : {&w->codes, &w->cls, &w->parent, &w->size, &w->first, &w->slot}) CNA_TRY(buf_need(c, st, *b, 4 * n));
  CNA_TRY(buf_need(c, st, w->hubs, 4 * hub_cap));
  CNA_TRY(buf_need(c, st, w->ctr, 8 * CC_COUNTERS));
  CNA_TRY(buf_need(c, st, w->totals, 8 * (int64_t)n_classes));
  CNA_TRY(buf_need(c, st, w->list, 4 * 3 * n));
  // whatever the main stream has queued on the graph (a renumbering) comes first; this entry returns only after its own
  // stream has drained
  HIP_TRY(hipEventRecord(es->x_ready, c->stream));
  HIP_TRY(hipStreamWaitEvent(st, es->x_ready, 0));

  unsigned long long* ctr = w->ctr.as<unsigned long long>();
  int32_t* cls = w->cls.as<int32_t>();
  int32_t* parent = w->parent.as<int32_t>();
  int32_t* hubs = w->hubs.as<int32_t>();
  const unsigned cell_blocks = (unsigned)((n + 255) / 256);
  const unsigned row_blocks = (unsigned)std::min<int64_t>((n + 256 / CC_SUB - 1) / (256 / CC_SUB), CC_MAX_GRID);
  std::optional<ProfScope> span;
  span.emplace(c, CNA_K_COMPONENTS_UPLOAD, st);
  HIP_TRY(hipMemcpyAsync(w->codes.p, codes, (size_t)(4 * n), hipMemcpyHostToDevice, st));
  span.reset();
  HIP_TRY(hipMemsetAsync(ctr, 0, 8 * CC_COUNTERS, st));
  HIP_TRY(hipMemsetAsync(w->totals.p, 0, 8 * (size_t)n_classes, st));
  hipLaunchKernelGGL(k_cc_init, dim3(cell_blocks), dim3(256), 0, st, w->codes.as<const int32_t>(), (const int64_t*)c->orig_idx, n,
                     n_classes, cls, parent, w->size.as<int32_t>(), w->first.as<int32_t>(), w->slot.as<int32_t>(), ctr);
  int round = 0;
  for (;;) {
    ++round;
    HIP_TRY(hipMemsetAsync(ctr, 0, 8 * 2, st));                     // the hub list and the count of open entries start over
    span.emplace(c, CNA_K_COMPONENTS_HOOK, st);
    int64_t done = 0;
    if (round == 1)
      for (; done < CC_SAMPLES; ++done) {               // one entry of every row, then flat trees for the next launch's finds
        hipLaunchKernelGGL(k_cc_rows<false>, dim3(row_blocks), dim3(256), 0, st, (const int64_t*)c->indptr,
                           (const int32_t*)c->indices, (const int32_t*)cls, parent, n, nnz, done, done + 1, hubs, hub_cap, ctr);
        hipLaunchKernelGGL(k_cc_flatten, dim3(cell_blocks), dim3(256), 0, st, (const int32_t*)cls, parent, n);
      }
    hipLaunchKernelGGL(k_cc_rows<false>, dim3(row_blocks), dim3(256), 0, st, (const int64_t*)c->indptr, (const int32_t*)c->indices,
                       (const int32_t*)cls, parent, n, nnz, done, CC_ALL, hubs, hub_cap, ctr);
    hipLaunchKernelGGL(k_cc_hubs<false>, dim3(CC_HUB_BLOCKS), dim3(256), 0, st, (const int64_t*)c->indptr,
                       (const int32_t*)c->indices, (const int32_t*)cls, parent, n, nnz, (const int32_t*)hubs, hub_cap, ctr);
    span.reset();
    span.emplace(c, CNA_K_COMPONENTS_FLATTEN, st);
    hipLaunchKernelGGL(k_cc_flatten, dim3(cell_blocks), dim3(256), 0, st, (const int32_t*)cls, parent, n);
    span.reset();
    span.emplace(c, CNA_K_COMPONENTS_CHECK, st);
    hipLaunchKernelGGL(k_cc_rows<true>, dim3(row_blocks), dim3(256), 0, st, (const int64_t*)c->indptr, (const int32_t*)c->indices,
                       (const int32_t*)cls, parent, n, nnz, (int64_t)0, CC_ALL, hubs, hub_cap, ctr);
    hipLaunchKernelGGL(k_cc_hubs<true>, dim3(CC_HUB_BLOCKS), dim3(256), 0, st, (const int64_t*)c->indptr,
                       (const int32_t*)c->indices, (const int32_t*)cls, parent, n, nnz, (const int32_t*)hubs, hub_cap, ctr);
    span.reset();
    unsigned long long ctr_h[CC_COUNTERS];
    CNA_TRY(fetch_results(st, "cna_graph_components_find", {{ctr_h, ctr, sizeof(ctr_h)}}));
    if (ctr_h[CC_C_BAD_CODE]) CNA_FAIL(CNA_EINVAL, "cna_graph_components_find: a code lies outside [-1, n_classes)");
    if (!ctr_h[CC_C_BAD_EDGES]) break;
    if (round == CC_MAX_ROUNDS)
      CNA_FAIL(CNA_ESTATE, "cna_graph_components_find: " + std::to_string(ctr_h[CC_C_BAD_EDGES]) + " entries still join two trees after " +
                               std::to_string(CC_MAX_ROUNDS) + " rounds");
  }
  span.emplace(c, CNA_K_COMPONENTS_TALLY, st);
  int32_t* list = w->list.as<int32_t>();
  hipLaunchKernelGGL(k_cc_tally, dim3(cell_blocks), dim3(256), 0, st, (const int32_t*)cls, (const int32_t*)parent,
                     (const int64_t*)c->orig_idx, n, w->size.as<int32_t>(), w->first.as<int32_t>());
  hipLaunchKernelGGL(k_cc_compact, dim3(cell_blocks), dim3(256), 0, st, (const int32_t*)cls, (const int32_t*)parent,
                     w->size.as<const int32_t>(), w->first.as<const int32_t>(), n, min_cells, w->totals.as<unsigned long long>(), ctr,
                     list, list + n, list + 2 * n, w->slot.as<int32_t>());
  span.reset();
  unsigned long long kept_h = 0;
  std::vector<unsigned long long> totals_h((size_t)n_classes);
  CNA_TRY(fetch_results(st, "cna_graph_components_find",
                        {{&kept_h, ctr + CC_C_KEPT, 8}, {totals_h.data(), w->totals.p, 8 * (size_t)n_classes}}));
  if ((int64_t)kept_h > n) CNA_FAIL(CNA_ESTATE, "cna_graph_components_find: more components than cells");
  for (int k = 0; k < n_classes; ++k) totals_out[k] = (int64_t)totals_h[(size_t)k];
  *n_kept_out = (int64_t)kept_h;
  *sweeps_out = round;
  w->n = n;
  w->kept = (int64_t)kept_h;
  w->indptr = c->indptr;
  w->orig = c->orig_idx;
  return 0;
}

extern "C" int cna_graph_components_list(cna_ctx* c, int64_t n_kept, int32_t* class_out, int32_t* size_out, int32_t* first_out) {
  CHECK_CTX(c);
  ExprState* es = nullptr;
  ComponentsWork* w = nullptr;
  CNA_TRY(cc_work(c, "cna_graph_components_list", -1, n_kept, &es, &w));
  if (n_kept == 0) return 0;
  if (!class_out || !size_out || !first_out) CNA_FAIL(CNA_EINVAL, "cna_graph_components_list: null pointer");
  ProfScope ps(c, CNA_K_COMPONENTS_FETCH, es->st);
  const int32_t* list = w->list.as<const int32_t>();
  const size_t bytes = 4 * (size_t)n_kept;
  return fetch_results(es->st, "cna_graph_components_list",
                       {{class_out, list, bytes}, {size_out, list + w->n, bytes}, {first_out, list + 2 * w->n, bytes}});
}

extern "C" int cna_graph_components_label(cna_ctx* c, const int32_t* rank, int64_t n_kept, int32_t* comp_out, int64_t n_cells) {
  CHECK_CTX(c);
  if (!comp_out) CNA_FAIL(CNA_EINVAL, "cna_graph_components_label: null pointer");
  ExprState* es = nullptr;
  ComponentsWork* w = nullptr;
  CNA_TRY(cc_work(c, "cna_graph_components_label", n_cells, n_kept, &es, &w));
  hipStream_t st = es->st;
  const int64_t n = w->n;
  if (rank)
    for (int64_t j = 0; j < n_kept; ++j)
      if (rank[j] < 0 || rank[j] >= n_kept) CNA_FAIL(CNA_EINVAL, "cna_graph_components_label: a rank lies outside [0, n_kept)");
  CNA_TRY(buf_need(c, st, w->comp, 4 * n));
  if (rank && n_kept) {
    CNA_TRY(buf_need(c, st, w->rank, 4 * n_kept));
    HIP_TRY(hipMemcpyAsync(w->rank.p, rank, (size_t)(4 * n_kept), hipMemcpyHostToDevice, st));
  }
  {
    ProfScope ps(c, CNA_K_COMPONENTS_LABEL, st);
    HIP_TRY(hipMemsetAsync(w->comp.p, 0xff, (size_t)(4 * n), st));  // (a cell order that names a cell twice leaves another at -1)
    hipLaunchKernelGGL(k_cc_label, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w->cls.as<const int32_t>(),
                       w->parent.as<const int32_t>(), w->slot.as<const int32_t>(),
                       rank && n_kept ? w->rank.as<const int32_t>() : (const int32_t*)nullptr, n_kept, (const int64_t*)c->orig_idx, n,
                       w->comp.as<int32_t>());
  }
  ProfScope ps(c, CNA_K_COMPONENTS_FETCH, st);
  return fetch_results(st, "cna_graph_components_label", {{comp_out, w->comp.p, 4 * (size_t)n}});
}

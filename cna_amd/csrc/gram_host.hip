// The Gram matrix X^T X and the global F-tests on the host (extern "C" entry points of libcna_hip.so, see include/cna_hip.h):
// what is queued around the kernels of mfma.hip and stats.hip, and how their results reach the host.
#include "common.h"
#include <chrono>
#include <cmath>
#include <cstring>

// ---- the Gram matrix under the walk's last step (see common.h: gram_pre) -------------------------------------
// CNA_GRAM_OVERLAP = K: the step that leaves the selection by-product runs in K row ranges (0 / 1: one launch, the
// Gram kernel afterwards as before).  Measured on C4 (profiles/r04_ab_gram_overlap.txt): without stream priorities the
// Gram ranges take the chip whenever they become ready and the step grows by what they take; with priorities, or with
// the two sides confined to disjoint CUs (hipExtStreamCreateWithCUMask), nothing is gained either -- the gather is bound
// per CU and a Gram workgroup displaces the walk waves of the CU it lands on.  Off by default; the switch stays for the
// bit-identity test of the ranged product.
int gram_overlap_ranges() {
  const char* e = getenv("CNA_GRAM_OVERLAP");
  const int k = e ? atoi(e) : 0;
  return k < 0 ? 0 : (k > 64 ? 64 : k);
}
int ensure_gram_stream(cna_ctx* c) {
  if (c->gram_stream_state) return c->gram_stream_state;
  c->gram_stream_state = -1;
  hipError_t err = hipStreamCreateWithFlags(&c->gram_stream, hipStreamNonBlocking);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&c->gram_pre_done, hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&c->range_done, hipEventDisableTiming);
  if (err != hipSuccess) { (void)hipGetLastError(); return -1; }
  c->gram_stream_state = 1;
  return 1;
}
// The Gram matrix reaches the host without a copy engine (round 6): its reduction kernel writes it a second time into
// pinned memory (one rank), or a copy kernel behind the ranks' sum does.  An asynchronous copy from another stream sat
// in the engine's queue behind the per-cell columns of the same analysis: 2 ms at 2M cells (cna_assoc_out.t_ms[9]).
int gram_host_reserve(cna_ctx* c, int Nx) {
  const int64_t bytes = (int64_t)sizeof(double) * Nx * Nx;
  if (bytes > c->h_gram_cap) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->h_gram) HIP_TRY(hipHostFree(c->h_gram));
    c->h_gram = nullptr;
    c->h_gram_cap = 0;
    HIP_TRY(hipHostMalloc(&c->h_gram, (size_t)bytes, hipHostMallocDefault));
    c->h_gram_cap = bytes;
  }
  return 0;
}
bool gram_solo(cna_ctx* c) { return !(c->nranks > 1 || comm_active(c)); }
int gram_host_finish(cna_ctx* c, int Nx) {      // behind the reduction (and the ranks' sum): G on the host when gram_done fires
  if (!c->gram_mirrored) CNA_TRY(launch_copy_f64(c, c->gram_buf, (double*)c->h_gram, (int64_t)Nx * Nx));
  HIP_TRY(hipEventRecord(c->gram_done, c->stream));
  c->gram_n = Nx;
  return 0;
}
// whoever is about to write c->gram_buf / c->gram_part on another stream, or to start the next ranged product
int gram_pre_settle(cna_ctx* c) {
  if (c->gram_pre_pending) {
    HIP_TRY(hipStreamWaitEvent(c->stream, c->gram_pre_done, 0));
    c->gram_pre_pending = false;
  }
  return 0;
}

int gram_launch_now(cna_ctx* c) {
  const int Nx = c->Nx;
  const bool pre = c->gram_pre && c->gram_pre_pending;     // taken under the walk's last step (ranged_last_step), X untouched since
  c->gram_pre = false;
  CNA_TRY(gram_pre_settle(c));
  CNA_TRY(gram_host_reserve(c, Nx));
  c->gram_mirrored = false;
  if (!pre) {
    void* g = c->gram_buf;
    CNA_TRY(dev_reserve(c, &g, &c->gram_cap, (int64_t)sizeof(double) * Nx * Nx));
    c->gram_buf = (double*)g;
    c->gram_mirror = gram_solo(c) ? (double*)c->h_gram : nullptr;
    const int rc = launch_gram(c, c->gram_buf);
    c->gram_mirror = nullptr;
    CNA_TRY(rc);
  }
  CNA_TRY(comm_allreduce_f64_sum(c, c->gram_buf, (size_t)Nx * Nx));
  return gram_host_finish(c, Nx);
}

extern "C" {

int cna_gram_launch(cna_ctx* c) {
  CHECK_CTX(c);
  if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "X not available");
  return gram_launch_now(c);
}

// Only waits for the event and reads the pinned copy: safe to call while another host thread is blocked inside a
// long entry point of the same context (cna_null_local_resident).
int cna_gram_fetch(cna_ctx* c, double* G_out) {
  CHECK_CTX(c);
  if (c->gram_n < 1) CNA_FAIL(CNA_ESTATE, "cna_gram_fetch before cna_gram_launch");
  const int64_t bytes = (int64_t)sizeof(double) * c->gram_n * c->gram_n;
  HIP_TRY(hipEventSynchronize(c->gram_done));
  std::memcpy(G_out, c->h_gram, (size_t)bytes);
  return 0;
}

// Gram matrix -> leading eigenpairs -> F-tests queued, without the interpreter in between (round 5): what follows the
// Gram kernels on the critical path of a small block is sample-space work of ~0.5 ms, and three trips through Python
// between its pieces cost a fifth of that again.  The acceptance rule of the native pairs is tools/_nam.py's
// (_top_pcs_native): residual and orthogonality at rounding level, every leading gap wide enough for the individual
// vectors to be defined; otherwise *accepted = 0 and the caller takes LAPACK (G_out is valid either way).
int cna_gram_pcs_tests(cna_ctx* c, int kmax, const int32_t* ks, int K, int r, int use_native, double resid_tol, double gap_tol,
                       double* G_out, double* U_out, int* accepted) {
  CHECK_CTX(c);
  if (!G_out || !U_out || !accepted || !ks) CNA_FAIL(CNA_EINVAL, "cna_gram_pcs_tests: null argument");
  *accepted = 0;
  CNA_TRY(cna_gram_fetch(c, G_out));
  c->t_gram_fetched = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
  const int n = c->gram_n;
  if (!use_native || n < 8 || kmax < 1 || 4 * kmax > n || kmax + 1 > 256) return 0;
  for (int64_t i = 0; i < (int64_t)n * n; ++i)
    if (!std::isfinite(G_out[i])) return 0;
  std::vector<double> lam((size_t)kmax + 1);
  double resid = 0.0, ortho = 0.0;
  if (cna_host_top_eig(G_out, n, kmax, U_out, lam.data(), &resid, &ortho) != 0) return 0;
  const double top = lam[0];
  if (!(top > 0.0)) return 0;
  for (int t = 0; t <= kmax; ++t)
    if (!std::isfinite(lam[t])) return 0;
  if (!(resid <= resid_tol * top && ortho <= resid_tol)) return 0;
  for (int t = 0; t < kmax; ++t)
    if (!(lam[t] - lam[t + 1] > gap_tol * top)) return 0;
  CNA_TRY(cna_global_test_launch(c, U_out, kmax, ks, K, r));
  *accepted = 1;
  return 0;
}

int cna_gram(cna_ctx* c, double* G_out) {
  CNA_TRY(cna_gram_launch(c));
  return cna_gram_fetch(c, G_out);
}

// The global F-tests in two halves: launch stages U and ks in pinned memory, queues upload, kernels
// and the copy of the three result vectors back into the pinned block on the second stream, and
// returns; fetch waits for them.  The caller can do host work (write the coefficient column) between.
int cna_global_test_launch(cna_ctx* c, const double* U, int kmax, const int32_t* ks, int K, int r) {
  CHECK_CTX(c);
  if (!c->zc || c->zc_cols < 1 || c->zc_rows != c->Nx) CNA_FAIL(CNA_ESTATE, "cna_global_test needs cna_condition_phenotypes");
  const int N = c->Nx, P = c->zc_cols;
  if (kmax < 1 || kmax > N || K < 1) CNA_FAIL(CNA_EINVAL, "cna_global_test: bad kmax / K");
  for (int a = 0; a < K; ++a)
    if (ks[a] < 1 || ks[a] > kmax) CNA_FAIL(CNA_EINVAL, "cna_global_test: ks must lie in [1, kmax]");
  if (c->gt_pending_P) CNA_FAIL(CNA_ESTATE, "a global test is still pending: fetch it first");
  void* g = c->gt;
  const int64_t nwork = global_test_scratch_doubles(P, kmax, K);
  CNA_TRY(dev_reserve(c, &g, &c->gt_cap, carve_bytes({8 * (int64_t)N * kmax, 4 * (int64_t)K, 8 * (int64_t)P, 8 * (int64_t)P, 4 * (int64_t)P, 8 * nwork})));
  c->gt = g;
  Carver cv(c->gt);
  double* Ud = cv.take<double>((int64_t)N * kmax);
  int32_t* ksd = cv.take<int32_t>(K);
  double* mp = cv.take<double>(P);
  double* r2 = cv.take<double>(P);
  int32_t* ki = cv.take<int32_t>(P);
  double* work = cv.take<double>(nwork);
  const int64_t off_ks = 8 * (int64_t)N * kmax;
  const int64_t off_out = round_up(off_ks + 4 * (int64_t)K, 64);
  const int64_t need = off_out + 20 * (int64_t)P + 64;
  if (need > c->h_gt_cap) {
    if (c->h_gt) HIP_TRY(hipHostFree(c->h_gt));
    c->h_gt = nullptr;
    HIP_TRY(hipHostMalloc(&c->h_gt, (size_t)need, hipHostMallocDefault));
    c->h_gt_cap = need;
  }
  char* h = (char*)c->h_gt;
  std::memcpy(h, U, 8 * (size_t)N * kmax);
  std::memcpy(h + off_ks, ks, 4 * (size_t)K);
  // Runs on the copy stream: Zc is complete (cna_condition_phenotypes synchronised) and only read, so
  // these tiny kernels need not queue behind a local-null pass in flight on the main stream.
  hipStream_t st = c->copy_stream;
  HIP_TRY(hipMemcpyAsync(Ud, h, 8 * (size_t)N * kmax, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ksd, h + off_ks, 4 * (size_t)K, hipMemcpyHostToDevice, st));
  CNA_TRY(launch_global_test(c, st, c->zc, c->zc_ld, N, P, Ud, kmax, ksd, K, r, work, mp, r2, ki));
  HIP_TRY(hipMemcpyAsync(h + off_out, mp, 8 * (size_t)P, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h + off_out + 8 * (size_t)P, r2, 8 * (size_t)P, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h + off_out + 16 * (size_t)P, ki, 4 * (size_t)P, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(c->gt_done, st));
  c->gt_pending_P = P;
  c->gt_off_out = off_out;
  return 0;
}

int cna_global_test_fetch(cna_ctx* c, double* minp_out, double* r2_out, int32_t* kidx_out) {
  CHECK_CTX(c);
  if (!c->gt_pending_P) CNA_FAIL(CNA_ESTATE, "no global test pending");
  const size_t P = (size_t)c->gt_pending_P;
  c->gt_pending_P = 0;
  HIP_TRY(hipEventSynchronize(c->gt_done));
  const char* o = (const char*)c->h_gt + c->gt_off_out;
  if (minp_out) std::memcpy(minp_out, o, 8 * P);
  if (r2_out) std::memcpy(r2_out, o + 8 * P, 8 * P);
  if (kidx_out) std::memcpy(kidx_out, o + 16 * P, 4 * P);
  return 0;
}

int cna_global_test(cna_ctx* c, const double* U, int kmax, const int32_t* ks, int K, int r, double* minp_out,
                    double* r2_out, int32_t* kidx_out) {
  CNA_TRY(cna_global_test_launch(c, U, kmax, ks, K, r));
  return cna_global_test_fetch(c, minp_out, r2_out, kidx_out);
}

}  // extern "C"

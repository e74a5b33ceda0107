// The selection pass's row standardisation, stated once (device code only): NAM row -> row of X, its coefficient
// X.y/N, its digit planes for the integer local null, and the running max |coefficient| of a workgroup.  Used by
// rows.hip (k_select_std, k_select_std16, k_standardize, k_resid_lowrank, k_ncorrs), diffuse.hip (select_tail),
// mfma.hip (k_selgram_blk) and rows16.hip (k_rowpass16).
//
// Floating-point contraction: this header sets NO contraction pragma.  Its functions compile under the mode of the file
// that includes them -- rows.hip and mfma.hip contract (`ss += d * d`, `dot += y * x` and the row scale are FMAs there),
// diffuse.hip includes it BELOW its `#pragma clang fp contract(off)` (a multiply, then an add).  That is why the walk's
// by-product agrees with the separate pass to rounding and not bit for bit, and it has to stay so.  Everything is
// therefore local to the including file (anonymous namespace).
#pragma once
#include "common.h"

namespace {

// ---- lane groups: who shares a row, how its lanes reduce, who speaks for it
struct Wave64 {   // one row per wave
  __device__ __forceinline__ static double sum(double v) { return wave_sum(v); }
  __device__ __forceinline__ static double max(double v) { return wave_max_d(v); }
  __device__ __forceinline__ static bool leader(int lane) { return lane == 0; }
  __device__ __forceinline__ static bool all(bool p, int) { return __all(p); }
};
struct Row16 {    // four rows per wave, sixteen lanes each
  __device__ __forceinline__ static double sum(double v) { return row16_sum(v); }
  __device__ __forceinline__ static double max(double v) { return row16_max(v); }
  __device__ __forceinline__ static bool leader(int lane) { return (lane & 15) == 0; }
  __device__ __forceinline__ static bool all(bool p, int lane) {
    const unsigned long long rowmask = 0xffffull << (16 * (lane >> 4));
    return (__ballot(p) & rowmask) == rowmask;
  }
};

// ---- column maps: element k of lane `lane` is column col(lane, k)
struct ColStride1 {   // one double per lane: col = lane + 64*k
  __device__ __forceinline__ static int col(int lane, int k) { return lane + 64 * k; }
};
struct ColPair {      // double2 per lane: cols 2*(lane + 64*(k/2)) + (k&1)
  __device__ __forceinline__ static int col(int lane, int k) { return 2 * (lane + 64 * (k >> 1)) + (k & 1); }
};
struct ColQuad {      // four adjacent columns per lane (4-byte state: one float4): cols 4*(lane + 64*(k/4)) + (k&3)
  __device__ __forceinline__ static int col(int lane, int k) { return 4 * (lane + 64 * (k >> 2)) + (k & 3); }
};
struct ColQuad16 {    // sixteen lanes per row, four adjacent columns per lane and group of 64: cols 64*(k/4) + 4*l16 + (k&3)
  __device__ __forceinline__ static int col(int lane, int k) { return 64 * (k >> 2) + 4 * (lane & 15) + (k & 3); }
};

// ---- std with ddof = 1 the way pandas takes it: avg = sum/N ; sqrt(sum((avg-x)^2)/(N-1)).  `sum`: this lane's share of sum(x)
template <class LG, class CM, int NE>
__device__ __forceinline__ double row_sd(const double (&x)[NE], double sum, int lane, int Nx) {
  const double n = (double)Nx;
  const double avg = LG::sum(sum) / n;
  double ss = 0.0;
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    if (CM::col(lane, e) < Nx) {
      const double d = avg - x[e];
      ss += d * d;
    }
  }
  return sqrt(LG::sum(ss) / (n - 1.0));
}

// ---- the row pass.  x[]: the lane's elements of the selected NAM row (zero beyond Nx and in rows that are not live),
// sum: their sum; on return the row of X.  A row in which pandas sees zero variance (avg = sum/N, every avg - x == 0;
// _association.py:182) is counted in *nzero if it is live.  Returns this lane's share of max |x| and of X.y:
// ydot(dot, e, xs) adds element e's term y[col] * xs to dot (the caller has y in registers, or loads it where the column
// exists).  proj(x) sits between the centring (_nam.py:122) and the std of the centred values (_nam.py:159):
// NoProjector, or k_select_std's x <- x - (x.W^T).C^T.
struct RowStd {
  double amax, dot;
};
struct NoProjector {
  template <int NE>
  __device__ __forceinline__ void operator()(double (&)[NE]) const {}
};
template <class LG, class CM, int NE, class Proj, class YDot>
__device__ __forceinline__ RowStd row_standardize(double (&x)[NE], double sum, int lane, int Nx, bool live,
                                                  unsigned long long* nzero, const Proj& proj, const YDot& ydot) {
  const double avg0 = LG::sum(sum) / (double)Nx;
  bool flat = true;
#pragma unroll
  for (int e = 0; e < NE; ++e)
    if (CM::col(lane, e) < Nx) flat = flat && (avg0 - x[e] == 0.0);
  if (LG::all(flat, lane) && live && LG::leader(lane)) atomicAdd(nzero, 1ull);
#pragma unroll
  for (int e = 0; e < NE; ++e)
    if (CM::col(lane, e) < Nx) x[e] -= avg0;
  proj(x);
  double s2 = 0.0;
#pragma unroll
  for (int e = 0; e < NE; ++e) s2 += x[e];
  const double sd = row_sd<LG, CM>(x, s2, lane, Nx);
  RowStd o = {0.0, 0.0};
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const double xs = CM::col(lane, e) < Nx ? __ddiv_rn(x[e], sd) : 0.0;
    x[e] = xs;
    ydot(o.dot, e, xs);
    o.amax = fmax(o.amax, fabs(xs));                      // NaN rows (zero variance): fmax drops them, q = 0 below
  }
  return o;
}

// ---- digit planes of the integer local null (null_i8.hip: [row][digit][Kp] bytes, one scale per row)
__device__ __forceinline__ double i8_inv(double rmax) { return rmax > 0.0 ? I8_QMAX / rmax : 0.0; }
__device__ __forceinline__ void i8_bytes(double x, double inv, unsigned& d0, unsigned& d1, unsigned& d2) {
  const double v = x * inv;
  digits3(v == v ? (int)rint(v) : 0, d0, d1, d2);
}
// J adjacent values -> their bytes in the low J bytes of one word per plane
template <int J>
__device__ __forceinline__ void i8_pack(const double* x, double inv, unsigned& w0, unsigned& w1, unsigned& w2) {
  w0 = w1 = w2 = 0;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    unsigned d0, d1, d2;
    i8_bytes(x[j], inv, d0, d1, d2);
    w0 |= d0 << (8 * j);
    w1 |= d1 << (8 * j);
    w2 |= d2 << (8 * j);
  }
}
// {max |x|, bound on sum |q|}: no reduction -- the row has sum x^2 = N - 1, so sum |x| < N and sum |q| <= N Q / max|x| + N / 2
__device__ __forceinline__ double2 i8_row_scale(double rmax, double n) {
  return make_double2(rmax, rmax > 0.0 ? n * (I8_QMAX / rmax) + n : 0.0);
}
// How a layout stores its bytes (rq: the row's planes).  Four adjacent columns per lane (ColQuad, ColQuad16): one dword
// per plane.  k_select_std's one column per lane meets in LDS first: that store stays with the kernel.
template <class CM, int NE>
__device__ __forceinline__ void store_planes(CM, const double (&x)[NE], double inv, int lane, unsigned char* rq, int Kp, bool live) {
#pragma unroll
  for (int k = 0; k < NE; k += 4) {
    unsigned w0, w1, w2;
    i8_pack<4>(&x[k], inv, w0, w1, w2);
    const int c0 = CM::col(lane, k);
    if (live && c0 < Kp) {
      *(unsigned*)(rq + c0) = w0;
      *(unsigned*)(rq + Kp + c0) = w1;
      *(unsigned*)(rq + 2 * Kp + c0) = w2;
    }
  }
}
// ColPair: a lane has two bytes of each plane; even lanes store dwords, their own half and the odd neighbour's
template <int NE>
__device__ __forceinline__ void store_planes(ColPair, const double (&x)[NE], double inv, int lane, unsigned char* rq, int Kp, bool) {
#pragma unroll
  for (int k = 0; k < NE; k += 2) {
    unsigned h0, h1, h2;
    i8_pack<2>(&x[k], inv, h0, h1, h2);
    const unsigned p01 = h0 | (h1 << 16);
    const unsigned o01 = (unsigned)__builtin_amdgcn_ds_bpermute(4 * (lane + 1), (int)p01);
    const unsigned o2 = (unsigned)__builtin_amdgcn_ds_bpermute(4 * (lane + 1), (int)h2);
    const int c0 = ColPair::col(lane, k);
    if ((lane & 1) == 0 && c0 < Kp) {
      *(unsigned*)(rq + c0) = (p01 & 0xffffu) | (o01 << 16);
      *(unsigned*)(rq + Kp + c0) = (p01 >> 16) | (o01 & 0xffff0000u);
      *(unsigned*)(rq + 2 * Kp + c0) = (h2 & 0xffffu) | (o2 << 16);
    }
  }
}

// ---- the running max |coefficient|.  Non-negative doubles order like their bit patterns; NaN (0x7ff8...) sorts above +inf
__device__ __forceinline__ void coef_note(double v, double& vmax, bool& any_nan) {
  const double av = fabs(v);
  if (av > vmax) vmax = av;
  any_nan = any_nan || (v != v);
}
__device__ __forceinline__ unsigned long long coef_max_bits(double vmax, bool any_nan) {
  return any_nan ? 0x7ff8000000000000ull : (unsigned long long)__double_as_longlong(vmax);
}
// End of a kernel of NW waves: one slot per workgroup, folded by k_max_fold (8192 same-address atomics cost ~80 us).
// wmax: NW words of LDS.  ACROSS: the lanes of a wave hold different rows' values (the 16-lane kernels) and meet here.
template <int NW, bool ACROSS>
__device__ __forceinline__ void coef_max_epilogue(unsigned long long* wmax, int lane, int wv, double vmax, bool any_nan,
                                                  unsigned long long* __restrict__ blockmax) {
  if (ACROSS) {
    any_nan = __any(any_nan);
    vmax = wave_max_d(vmax);
  }
  if (lane == 0) wmax[wv] = coef_max_bits(vmax, any_nan);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long m = wmax[0];
    for (int i = 1; i < NW; ++i) m = wmax[i] > m ? wmax[i] : m;
    blockmax[blockIdx.x] = m;
  }
}

}  // namespace

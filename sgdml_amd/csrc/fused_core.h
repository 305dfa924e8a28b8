// The single-launch predictor, written once: descriptor, double-buffered row loop, four-wavefront partial, ticket, ordered
// partial sum, Jacobian and back-projection of ONE geometry per workgroup column (grid = (row shares, geometries)).
// Used by predict_fused_kernel (predict.hip: geometry in the kernel arguments, results through host-mapped memory),
// md_step_kernel (md.hip) and relax_step_kernel (relax.hip: geometry in LDS, results into the device state).  The three
// produce the same bits for the same geometry: tests/test_md_gpu.py and tests/test_relax_gpu.py assert it.
#pragma once
#include <math.h>

#include "common.h"

#define FUSED_MAX_Q 8    // geometries of one launch
#define FUSED_MAX_N3 72  // coordinates of a geometry held in LDS: 3 N for D = N (N - 1) / 2 <= 256, N <= 23

// model tables, row split and work buffers of a single launch
struct FusedModel {
  const double* xp;
  const double* jap;
  const double* aE;
  int64_t MP;
  int D, N;
  double sig;
  int rows_per_wave;
  double* part;       // (B, n_wg, D + 1) workgroup partials: F_x, then E
  unsigned* counter;  // [q] workgroups of geometry q that have finished; predict_fused_kernel: [FUSED_MAX_Q] geometries done
  Lattice L;
};

__device__ __forceinline__ void pair_of(int k, int& i, int& j) {  // k = i (i - 1) / 2 + j, i > j
  i = (int)((1.0 + sqrt(1.0 + 8.0 * (double)k)) * 0.5);
  while (i * (i - 1) / 2 > k) --i;
  while ((i + 1) * i / 2 <= k) ++i;
  j = k - i * (i - 1) / 2;
}

// r_i - r_j of the geometry r (N, 3) (minimum image with a lattice: desc.py:44-77, as desc.hip forms it).  RP: a pointer into
// the kernel-argument segment or into LDS.
template <class RP>
__device__ __forceinline__ void pair_diff(RP r, const Lattice& L, int i, int j, double (&d)[3]) {
  double d0 = r[3 * i] - r[3 * j], d1 = r[3 * i + 1] - r[3 * j + 1], d2 = r[3 * i + 2] - r[3 * j + 2];
  if (L.use) {
    const double c0 = rint(L.inv[0] * d0 + L.inv[1] * d1 + L.inv[2] * d2);
    const double c1 = rint(L.inv[3] * d0 + L.inv[4] * d1 + L.inv[5] * d2);
    const double c2 = rint(L.inv[6] * d0 + L.inv[7] * d1 + L.inv[8] * d2);
    d0 -= L.lat[0] * c0 + L.lat[1] * c1 + L.lat[2] * c2;
    d1 -= L.lat[3] * c0 + L.lat[4] * c1 + L.lat[5] * c2;
    d2 -= L.lat[6] * c0 + L.lat[7] * c1 + L.lat[8] * c2;
  }
  d[0] = d0; d[1] = d1; d[2] = d2;
}

// This workgroup's share for the geometry r of q = blockIdx.y: x from r into registers, its table rows into F_x and E, the
// four wavefronts summed through LDS into one partial, then the ticket.  True for the geometry's last workgroup, which goes
// on to fused_sum_partials.
template <int KPL, class RP>
__device__ __forceinline__ bool fused_partials(const FusedModel& A, RP r, double (&s_fx)[4][KPL * 64], double (&s_E)[4],
                                               unsigned& s_ticket) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = A.D;
  const int q = (int)blockIdx.y;  // a workgroup serves ONE geometry
  const double sig = A.sig, inv_sig = 1.0 / sig;
  const double sqrt5 = 2.23606797749978969641;
  const double fact = 5.0 / (3.0 * sig * sig * sig);
  const double dscale = 5.0 / sig;
  const double inv_3sig = 1.0 / (3.0 * sig);

  // ---- descriptor of the geometry (same arithmetic as desc_kernel)
  double x[KPL], Fx[KPL], E = 0.0;
#pragma unroll
  for (int t = 0; t < KPL; ++t) {
    const int k = lane + 64 * t;
    double v = 0.0;
    if (k < D) {
      int i, j;
      pair_of(k, i, j);
      double d[3];
      pair_diff(r, A.L, i, j, d);
      v = 1.0 / sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    }
    x[t] = v;
    Fx[t] = 0.0;
  }

  // ---- this wavefront's table rows (the row loop of predict_kernel)
  const int64_t gw = (int64_t)blockIdx.x * 4 + wave;
  const int64_t r0 = gw * A.rows_per_wave;
  const int64_t r1 = (r0 + A.rows_per_wave < A.MP) ? r0 + A.rows_per_wave : A.MP;
  const bool has_aE = A.aE != nullptr;
  auto load_row = [&](int64_t r, double (&X)[KPL], double (&JA)[KPL], double& ae) {
#pragma unroll
    for (int t = 0; t < KPL; ++t) {
      const int k = lane + 64 * t;
      const int kc = k < D ? k : D - 1;
      const double xv = __hip_atomic_load(A.xp + r * D + kc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      const double jv = __hip_atomic_load(A.jap + r * D + kc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      X[t] = (k < D) ? xv : 0.0;
      JA[t] = (k < D) ? jv : 0.0;
    }
    ae = has_aE ? __hip_atomic_load(A.aE + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) : 0.0;
  };
  auto row = [&](const double (&X)[KPL], const double (&JA)[KPL], double ae) {
    double d[KPL];
    double s2 = 0.0, sa = 0.0;
#pragma unroll
    for (int t = 0; t < KPL; ++t) {
      d[t] = x[t] - X[t];
      s2 += d[t] * d[t];
      sa += d[t] * JA[t];
    }
    s2 = wave_sum(s2);
    sa = wave_sum(sa);
    const double nrm = sqrt5 * sqrt(s2);
    const double ex = exp(-nrm * inv_sig);
    const double b = fact * ex;
    const double b2 = b * (nrm + sig);
    double w1 = dscale * sa * b;
    E += sa * b2;
    if (has_aE) {
      w1 += ae * b2;
      E += ae * (1.0 + (nrm * inv_sig) * (1.0 + nrm * inv_3sig)) * ex;
    }
#pragma unroll
    for (int t = 0; t < KPL; ++t) Fx[t] += w1 * d[t] - b2 * JA[t];
  };
  if (r0 < r1) {
    double X0[KPL], JA0[KPL], X1[KPL], JA1[KPL], ae0, ae1;
    int64_t r = r0;
    load_row(r, X0, JA0, ae0);
    for (; r + 1 < r1; r += 2) {
      load_row(r + 1, X1, JA1, ae1);
      row(X0, JA0, ae0);
      load_row(r + 2 < r1 ? r + 2 : r1 - 1, X0, JA0, ae0);
      row(X1, JA1, ae1);
    }
    if (r < r1) row(X0, JA0, ae0);
  }

  // ---- the workgroup's four wavefronts -> one partial (padding lanes hold zeros)
#pragma unroll
  for (int t = 0; t < KPL; ++t) s_fx[wave][lane + 64 * t] = Fx[t];
  if (lane == 0) s_E[wave] = E;
  __syncthreads();
  const int n_wg = (int)gridDim.x;
  double* my_part = A.part + ((int64_t)q * n_wg + blockIdx.x) * (D + 1);
  for (int k = tid; k < D; k += 256) my_part[k] = (s_fx[0][k] + s_fx[1][k]) + (s_fx[2][k] + s_fx[3][k]);
  if (tid == 0) my_part[D] = (s_E[0] + s_E[1]) + (s_E[2] + s_E[3]);
  __threadfence();
  __syncthreads();
  if (tid == 0) s_ticket = atomicAdd(A.counter + q, 1u);
  __syncthreads();
  return s_ticket == gridDim.x - 1;
}

// The geometry's last workgroup (every partial of the geometry is visible): the partials summed in a fixed order, F_x into
// fxs (D), E handed to put_E(double) by the one thread that holds it.
template <class PutE>
__device__ __forceinline__ void fused_sum_partials(const FusedModel& A, double* fxs, PutE&& put_E) {
  const int tid = threadIdx.x;
  const int D = A.D;
  const int n_wg = (int)gridDim.x;
  __threadfence();
  const double* qpart = A.part + (int64_t)blockIdx.y * n_wg * (D + 1);
  for (int k = tid; k < D + 1; k += 256) {
    double s = 0.0;
    for (int w0 = 0; w0 < n_wg; w0 += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int w = w0 + u < n_wg ? w0 + u : n_wg - 1;
        v[u] = __hip_atomic_load(qpart + (int64_t)w * (D + 1) + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (w0 + u < n_wg) s += v[u];
    }
    if (k < D) fxs[k] = s;
    else put_E(s);
  }
}

// Jacobian entries (r_i - r_j) / d^3 of the geometry r into s_g (D, 3)  (desc.py:193-205).  per_pair(k, d, inv3) runs in the
// thread that wrote fxs[k] in fused_sum_partials.  The caller synchronises the workgroup before fused_force.
struct FusedNoPair {
  __device__ __forceinline__ void operator()(int, const double (&)[3], double) const {}
};
template <class RP, class PerPair = FusedNoPair>
__device__ __forceinline__ void fused_jacobian(const FusedModel& A, RP r, double* s_g, PerPair&& per_pair = PerPair()) {
  for (int k = threadIdx.x; k < A.D; k += 256) {
    int i, j;
    pair_of(k, i, j);
    double d[3];
    pair_diff(r, A.L, i, j, d);
    const double dist = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const double inv3 = 1.0 / (dist * dist * dist);
    s_g[k * 3 + 0] = d[0] * inv3;
    s_g[k * 3 + 1] = d[1] * inv3;
    s_g[k * 3 + 2] = d[2] * inv3;
    per_pair(k, d, inv3);
  }
}

// coordinate t of F = J_x^T F_x  (desc.py:405-408) in the order of predict_epilogue_kernel
__device__ __forceinline__ double fused_force(int N, const double* s_g, const double* fxs, int t) {
  const int a = t / 3, al = t - 3 * a;
  double f = 0.0;
  for (int m = 0; m < N; ++m) {
    if (m == a) continue;
    const int k = pair_idx(a, m);
    const double v = s_g[k * 3 + al] * fxs[k];
    f += (a < m) ? v : -v;
  }
  return f;
}

// ---- host side -----------------------------------------------------------------------------------
struct FusedPlan {
  int rows;  // table rows per wavefront
  int n_wg;  // workgroups (of four wavefronts) per geometry
  int KPL;   // descriptor entries per lane: 1, 2 or 4
};

// the shapes a single launch serves
static inline bool fused_serves(const Model& md, int64_t B) { return B >= 1 && B <= FUSED_MAX_Q && md.D >= 1 && md.D <= 256; }

// option predict.fused_rows, doubled until at most 4 x 256 wavefronts remain (a few per CU: the launch is latency bound, not
// throughput bound)
static inline FusedPlan fused_plan(const gdml_ctx* ctx, const Model& md) {
  const int64_t MP = md.M * md.P;
  FusedPlan P;
  P.rows = ctx_opt_i(ctx, "predict.fused_rows", 16);
  if (P.rows < 2) P.rows = 2;
  while ((MP + P.rows - 1) / P.rows > 1024) P.rows *= 2;
  P.n_wg = (int)(((MP + P.rows - 1) / P.rows + 3) / 4);
  P.KPL = 1;
  while (P.KPL * 64 < md.D) P.KPL <<= 1;
  return P;
}

// doubles of the partials of B geometries
static inline int64_t fused_part_len(const Model& md, const FusedPlan& P, int64_t B) { return B * P.n_wg * (md.D + 1); }

static inline void fused_fill(FusedModel& F, const Model& md, const FusedPlan& P, const double* lat, const double* lat_inv,
                              double* part, unsigned* counter) {
  F.xp = md.xp;
  F.jap = md.jap;
  F.aE = md.has_aE ? md.aE : nullptr;
  F.MP = md.M * md.P;
  F.D = md.D;
  F.N = md.N;
  F.sig = md.sig;
  F.rows_per_wave = P.rows;
  F.part = part;
  F.counter = counter;
  memset(&F.L, 0, sizeof(F.L));
  if (lat && lat_inv) {
    memcpy(F.L.lat, lat, sizeof(F.L.lat));
    memcpy(F.L.inv, lat_inv, sizeof(F.L.inv));
    F.L.use = 1;
  }
}

// k1, k2, k4: the kernel's instances for KPL = 1, 2, 4
template <class Args>
static inline void fused_launch(const FusedPlan& P, int64_t B, hipStream_t st, void (*k1)(Args), void (*k2)(Args),
                                void (*k4)(Args), const Args& A) {
  void (*const k)(Args) = P.KPL == 1 ? k1 : (P.KPL == 2 ? k2 : k4);
  hipLaunchKernelGGL(k, dim3((unsigned)P.n_wg, (unsigned)B), dim3(256), 0, st, A);
}

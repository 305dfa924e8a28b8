// On-device molecular dynamics (gdml_md_run, gdml_md_noise; include/gdml_hip.h has the equations): positions, velocities
// and forces of B independent replicas stay in device memory for the whole run, the host sees recorded frames only.
//
// Two routes, the same arithmetic of a step on both, plain launches queued on the context's stream, stream order being the only
// dependency between steps:
//   single launch (D <= 256, at most 8 replicas): md_step_kernel, one kernel per step (see there)
//   general (every other shape; ring polymers, gdml_pimd_run at the end of this file, have their own two kernels on this
//   shape), three pieces per step:
//     md_pre_kernel   half kick, drift (Langevin: half drift, Ornstein-Uhlenbeck step with Philox noise, half drift)
//     gdml_predict_dev on the new positions -- the library's device prediction path as it is (its route selection, its kernels)
//     md_post_kernel  second half kick, kinetic energy of each replica by a fixed tree, frame write on a recording step
// The host synchronises once per chunk of frames (bounded in bytes and in queued steps), copies the chunk out and reads the
// per-replica "first non-finite step" flags.  fp64 throughout, no atomics on floating-point values: results do not depend on
// chunking, on record_every or on how a run is cut into continued runs.
// Geometry relaxation (gdml_relax_run, batched FIRE with per-replica convergence) is the last part of this file: the same two
// routes and the same chunked driver, with a per-replica status word the host reads at chunk ends.
#include <math.h>

#include "common.h"

// ---- Philox4x32-10 (Salmon et al., SC'11), key = (seed lo, seed hi), counter = (step lo, step hi, replica, block) -------------
struct Philox4 {
  uint32_t v[4];
};

__host__ __device__ static inline Philox4 philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2,
                                                        uint32_t c3) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  Philox4 o;
  o.v[0] = c0;
  o.v[1] = c1;
  o.v[2] = c2;
  o.v[3] = c3;
  return o;
}

// standard normal of coordinate `coord` of replica `rep` at absolute step `step`: block = coord / 4, the block's outputs
// (x0, x1) and (x2, x3) are two Box-Muller pairs, u = (x + 0.5) 2^-32 in (0, 1)
__device__ static inline double md_normal(uint64_t seed, uint64_t step, uint32_t rep, int64_t coord) {
  const Philox4 o = philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)(step >> 32), rep,
                                  (uint32_t)(coord >> 2));
  const int j = (int)(coord & 3);
  const double u0 = ((double)o.v[j & 2] + 0.5) * 2.3283064365386963e-10;
  const double u1 = ((double)o.v[(j & 2) + 1] + 0.5) * 2.3283064365386963e-10;
  const double rad = sqrt(-2.0 * log(u0));
  const double ang = 6.283185307179586 * u1;
  return (j & 1) ? rad * sin(ang) : rad * cos(ang);
}

struct MdConst {
  int64_t B;
  int n3;
  double dt, f_scale, c1, c2, kT;
  int thermostat;
  uint64_t seed;
};

// first half of step `step` for coordinate k of replica b (the same arithmetic on both routes): half kick, drift, and with the
// thermostat the Ornstein-Uhlenbeck step between two half drifts
__device__ __forceinline__ void md_first_half(const MdConst& C, double m, double f, int64_t step, int64_t b, int64_t k, double& r,
                                              double& v) {
  v = v + 0.5 * C.dt * (C.f_scale * f / m);
  if (C.thermostat) {
    r = r + 0.5 * C.dt * v;
    const double xi = md_normal(C.seed, (uint64_t)step, (uint32_t)b, k);
    v = C.c1 * v + C.c2 * sqrt(C.kT / m) * xi;
    r = r + 0.5 * C.dt * v;
  } else {
    r = r + C.dt * v;
  }
}

// one thread per coordinate: first half of step `step` (absolute index)
__global__ void __launch_bounds__(256) md_pre_kernel(MdConst C, const double* __restrict__ mass, double* __restrict__ R,
                                                     double* __restrict__ V, const double* __restrict__ F,
                                                     int64_t* __restrict__ bad, int64_t step) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C.B * C.n3) return;
  const int64_t b = i / C.n3;
  const int64_t k = i - b * C.n3;
  double v = V[i], r = R[i];
  md_first_half(C, mass[k / 3], F[i], step, b, k, r, v);
  R[i] = r;
  V[i] = v;
  // every thread of a replica that finds the flag unset writes the same value: no ordering needed
  if (!(isfinite(r) && isfinite(v)) && bad[b] < 0) bad[b] = step;
}

struct MdFrame {
  double *R, *V, *F, *E, *Ekin;  // slot of the frame to write in the chunk buffers (null: not recorded)
  int on;
};

// one workgroup per replica: second half kick, kinetic energy (per-thread partial sums in index order, then a fixed tree),
// non-finite check of the new forces, frame write
__global__ void __launch_bounds__(256) md_post_kernel(MdConst C, const double* __restrict__ mass, const double* __restrict__ R,
                                                      double* __restrict__ V, const double* __restrict__ F,
                                                      const double* __restrict__ E, double* __restrict__ Ekin,
                                                      int64_t* __restrict__ bad, int64_t step, MdFrame fr) {
  __shared__ double red[256];
  __shared__ int nonfinite;
  const int64_t b = blockIdx.x;
  const int64_t o = b * C.n3;
  const int t = threadIdx.x;
  if (t == 0) nonfinite = 0;
  __syncthreads();
  double ek = 0.0;
  int nf = 0;
  for (int k = t; k < C.n3; k += 256) {
    const double m = mass[k / 3];
    const double f = F[o + k];
    const double v = V[o + k] + 0.5 * C.dt * (C.f_scale * f / m);
    V[o + k] = v;
    ek += 0.5 * m * v * v;
    nf |= !(isfinite(v) && isfinite(f));
    if (fr.on) {
      if (fr.R) fr.R[o + k] = R[o + k];
      if (fr.V) fr.V[o + k] = v;
      if (fr.F) fr.F[o + k] = f;
    }
  }
  red[t] = ek;
  if (nf) nonfinite = 1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  if (t == 0) {
    const double e = E[b];
    Ekin[b] = red[0];
    if ((nonfinite || !isfinite(e)) && bad[b] < 0) bad[b] = step;
    if (fr.on) {
      fr.E[b] = e;
      fr.Ekin[b] = red[0];
    }
  }
}

// ------------------------------------------------------------------------------------------
// Single-launch step for the shapes of the single-launch predictor (D <= 256, B <= 8 replicas): ONE kernel per step, modelled
// on predict_fused_kernel (predict.hip) -- the same row loop, row split, partial sums and back-projection order -- except that
//   - the state (R, V, F) of step t comes from device memory (one half of a ping-pong buffer), not from the kernel arguments;
//   - every workgroup of a replica redoes the cheap first half of the step (md_first_half) to hold r_{t+1} in LDS.
// grid = (row shares, replicas).  The LAST workgroup of a replica to finish (ticket) sums that replica's partials in a fixed
// order, forms F_{t+1} = J^T F_x, finishes the velocity, sums the kinetic energy by the tree of md_post_kernel and writes
// R, V, F, E', E_kin of step t + 1 to the other half of the state buffer (and to the frame slot on a recording step).  No
// workgroup reads what another workgroup of the same launch writes; stream order is the only dependency between steps.
// init: no kick and no drift -- the forces of the start geometry by the same arithmetic, so that a continued run starts from
// the bits the run it continues ended with.
// ------------------------------------------------------------------------------------------
#define MD_STEP_MAX_Q 8
#define MD_STEP_MAX_COORDS 72  // 3 N for D = N (N - 1) / 2 <= 256: N <= 23
// model tables, row split and work buffers of a single-launch step (md_step_kernel and relax_step_kernel)
struct StepModel {
  const double* xp;
  const double* jap;
  const double* aE;
  int64_t MP;
  int D, N;
  double sig;
  int rows_per_wave;
  double* part;       // (B, n_wg, D + 1) workgroup partials: F_x, then E
  unsigned* counter;  // [q] workgroups of replica q that have finished
  Lattice L;
};
struct MdStepArgs {
  StepModel M;
  int init;
  MdConst C;
  const double* mass;
  const double *inR, *inV, *inF;
  double *outR, *outV, *outF, *outE, *outEk;
  int64_t* bad;
  int64_t step;
  MdFrame fr;
};

// r_i - r_j (minimum image with a lattice, as desc.hip and predict_fused_kernel form it) from the LDS copy of one replica
__device__ __forceinline__ void md_pair_diff(const double* r, const Lattice& L, int i, int j, double (&d)[3]) {
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
__device__ __forceinline__ void md_pair_of(int k, int& i, int& j) {  // k = i (i - 1) / 2 + j, i > j
  i = (int)((1.0 + sqrt(1.0 + 8.0 * (double)k)) * 0.5);
  while (i * (i - 1) / 2 > k) --i;
  while ((i + 1) * i / 2 <= k) ++i;
  j = k - i * (i - 1) / 2;
}

// The predictor's share of a single-launch step, for the geometry s_r (LDS) of replica q = blockIdx.y: this workgroup's table
// rows into its partial, then the ticket.  True for the replica's last workgroup, which goes on to step_gather.
template <int KPL>
__device__ __forceinline__ bool step_partials(const StepModel& A, const double* s_r, double (&s_fx)[4][KPL * 64], double (&s_E)[4],
                                              unsigned& s_ticket) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = A.D;
  const int q = (int)blockIdx.y;  // a workgroup serves ONE replica
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
      md_pair_of(k, i, j);
      double d[3];
      md_pair_diff(s_r, A.L, i, j, d);
      v = 1.0 / sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    }
    x[t] = v;
    Fx[t] = 0.0;
  }

  // ---- this wavefront's table rows (the row loop of predict_fused_kernel)
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

// The replica's last workgroup (every partial of the replica is visible): the partials summed in the predictor's order into
// fxs (D) and s_Eq, and the Jacobian entries of s_r into s_g (D, 3).  step_force then back-projects one coordinate.
__device__ __forceinline__ void step_gather(const StepModel& A, const double* s_r, double* fxs, double* s_g, double& s_Eq) {
  const int tid = threadIdx.x;
  const int D = A.D;
  const int q = (int)blockIdx.y;
  const int n_wg = (int)gridDim.x;
  __threadfence();
  const double* qpart = A.part + (int64_t)q * n_wg * (D + 1);
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
    else s_Eq = s;
  }
  for (int k = tid; k < D; k += 256) {  // Jacobian entries (r_i - r_j) / d^3  (desc.py:193-205)
    int i, j;
    md_pair_of(k, i, j);
    double d[3];
    md_pair_diff(s_r, A.L, i, j, d);
    const double dist = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const double inv3 = 1.0 / (dist * dist * dist);
    s_g[k * 3 + 0] = d[0] * inv3;
    s_g[k * 3 + 1] = d[1] * inv3;
    s_g[k * 3 + 2] = d[2] * inv3;
  }
  __syncthreads();
}

// coordinate t of F = J_x^T F_x in the order of predict_epilogue_kernel
__device__ __forceinline__ double step_force(int N, const double* s_g, const double* fxs, int t) {
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

template <int KPL>
__global__ void __launch_bounds__(256) md_step_kernel(MdStepArgs A) {
  __shared__ double s_fx[4][KPL * 64];  // per-wavefront F_x; reused by the replica's last workgroup: [0] = its summed F_x
  __shared__ double s_E[4];
  __shared__ double s_g[KPL * 64 * 3];
  __shared__ double s_r[MD_STEP_MAX_COORDS], s_v[MD_STEP_MAX_COORDS];
  __shared__ double s_red[256];
  __shared__ double s_Eq;
  __shared__ unsigned s_ticket;
  __shared__ int s_nonfinite;
  const int tid = threadIdx.x;
  const int N = A.M.N, n3 = 3 * N;
  const int q = (int)blockIdx.y;  // a workgroup serves ONE replica

  // ---- first half of the step, redone by every workgroup of the replica: r_{t+1} and the half-kicked velocity into LDS
  if (tid < n3) {
    const int64_t o = (int64_t)q * n3 + tid;
    double r = A.inR[o], v = A.inV[o];
    if (!A.init) md_first_half(A.C, A.mass[tid / 3], A.inF[o], A.step, q, tid, r, v);
    s_r[tid] = r;
    s_v[tid] = v;
  }
  if (tid == 0) s_nonfinite = 0;
  __syncthreads();

  if (!step_partials<KPL>(A.M, s_r, s_fx, s_E, s_ticket)) return;
  double* fxs = &s_fx[0][0];
  step_gather(A.M, s_r, fxs, s_g, s_Eq);
  double ek = 0.0;
  if (tid < n3) {  // F = J_x^T F_x, then the second half kick
    const int t = tid, a = t / 3;
    const double f = step_force(N, s_g, fxs, t);
    const double m = A.mass[a];
    const double r = s_r[t];
    const double v = A.init ? s_v[t] : s_v[t] + 0.5 * A.C.dt * (A.C.f_scale * f / m);
    ek = 0.5 * m * v * v;
    const int64_t o = (int64_t)q * n3 + t;
    A.outR[o] = r;
    A.outV[o] = v;
    A.outF[o] = f;
    if (!(isfinite(r) && isfinite(v) && isfinite(f))) s_nonfinite = 1;
    if (A.fr.on) {
      if (A.fr.R) A.fr.R[o] = r;
      if (A.fr.V) A.fr.V[o] = v;
      if (A.fr.F) A.fr.F[o] = f;
    }
  }
  s_red[tid] = ek;  // the tree of md_post_kernel: the same kinetic energy bit for bit
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) s_red[tid] += s_red[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    const double e = s_Eq;
    A.outE[q] = e;
    A.outEk[q] = s_red[0];
    if ((s_nonfinite || !isfinite(e)) && A.bad[q] < 0) A.bad[q] = A.step;
    if (A.fr.on) {
      A.fr.E[q] = e;
      A.fr.Ekin[q] = s_red[0];
    }
    A.M.counter[q] = 0u;  // the next launch on the stream finds it reset
  }
}

__global__ void __launch_bounds__(256) md_noise_kernel(uint64_t seed, uint64_t step, int64_t B, int n3, double* __restrict__ xi) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * n3) return;
  const int64_t b = i / n3;
  xi[i] = md_normal(seed, step, (uint32_t)b, i - b * n3);
}

__global__ void __launch_bounds__(256) md_fill_i64_kernel(int64_t* p, int64_t n, int64_t v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// argument checks shared by every route; ctx may be NULL (the message then goes where gdml_ctx_create's goes)
static int md_check(gdml_ctx* ctx, const gdml_md_params* p, const double* R, const double* V, int64_t n_steps,
                    int64_t record_every) {
  if (!p) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: params is NULL");
  if (n_steps < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: n_steps < 0");
  if (record_every < 1) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: record_every < 1");
  if (p->B < 0 || p->B > 0x7fffffffLL) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: B out of range");
  if (p->N < 1 || p->N > GDML_MAX_ATOMS) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: N out of range");
  if (!(p->dt > 0.0) || !isfinite(p->dt)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: dt must be positive and finite");
  if (!isfinite(p->f_scale)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: f_scale is not finite");
  if (!p->mass) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: mass is NULL");
  for (int a = 0; a < p->N; ++a)
    if (!(p->mass[a] > 0.0) || !isfinite(p->mass[a]))
      return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: mass of atom %d must be positive and finite", a);
  if ((p->lat == nullptr) != (p->lat_inv == nullptr))
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: lattice and inverse must both be given or both NULL");
  if (p->thermostat != 0 && p->thermostat != 1)
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: thermostat must be 0 (none) or 1 (Langevin)");
  if (!(p->gamma >= 0.0) || !isfinite(p->gamma)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: gamma < 0");
  if (!(p->kT >= 0.0) || !isfinite(p->kT)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: kT < 0");
  if (p->step0 < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: step0 < 0");
  if (!R || !V) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: R or V is NULL");
  return GDML_OK;
}

// most bytes of frames, and most steps, queued between two synchronisations
static constexpr int64_t MD_CHUNK_BYTES = 64ll << 20;
static constexpr int64_t MD_CHUNK_STEPS = 4096;

extern "C" int gdml_md_run(gdml_ctx* ctx, const gdml_md_params* p, double* R, double* V, int64_t n_steps, int64_t record_every,
                           double* R_rec, double* V_rec, double* F_rec, double* E_rec, double* Ekin_rec,
                           int64_t* first_bad_step) {
  GDML_TRY(md_check(ctx, p, R, V, n_steps, record_every));
  if (!ctx) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: ctx is NULL");
  Model& md = ctx->model;
  if (!md.xp) return gdml_fail(ctx, GDML_ERR_STATE, "gdml_md_run: upload a model first");
  if (md.N != p->N) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: N = %d but the model has %d atoms", p->N, md.N);
  const int64_t B = p->B;
  const int n3 = 3 * p->N;
  if (first_bad_step)
    for (int64_t b = 0; b < B; ++b) first_bad_step[b] = -1;
  if (B == 0) return GDML_OK;
  HIP_CHECK(ctx, hipSetDevice(ctx->device));

  const int64_t nc = B * n3;
  const int64_t n_rec = n_steps / record_every;
  const int n_vec = (R_rec ? 1 : 0) + (V_rec ? 1 : 0) + (F_rec ? 1 : 0);
  const int64_t frame_bytes = (n_vec * nc + 2 * B) * 8;
  int64_t chunk_frames = MD_CHUNK_BYTES / frame_bytes;
  const int64_t opt = (int64_t)ctx_opt(ctx, "predict.md_chunk_frames", 0.0);
  if (opt > 0 && opt < chunk_frames) chunk_frames = opt;
  if (chunk_frames < 1) chunk_frames = 1;
  if (chunk_frames > n_rec) chunk_frames = n_rec;  // 0: nothing is recorded (n_steps < record_every)

  // the single-launch step serves the shapes of the single-launch predictor
  const int D = md.D;
  const bool fused = B <= MD_STEP_MAX_Q && D >= 1 && D <= 256 && n3 <= MD_STEP_MAX_COORDS && !ctx->profiling &&
                     ctx_opt_i(ctx, "predict.md_fused", 1) != 0;
  const int64_t MP = md.M * md.P;
  int rows = ctx_opt_i(ctx, "predict.fused_rows", 16);  // the row split of predict_fused: at most 4 x 256 wavefronts
  if (rows < 2) rows = 2;
  while ((MP + rows - 1) / rows > 1024) rows *= 2;
  const int n_wg = (int)(((MP + rows - 1) / rows + 3) / 4);

  // one allocation: mass | two halves of the state (R | V | F | E | Ekin each; the general route works in the first) | bad |
  // frames of a chunk (R, V, F as requested, E, Ekin) | workgroup partials and tickets of the single-launch step
  const int64_t n_half = 3 * nc + 2 * B;
  const int64_t n_state = p->N + 2 * n_half + B;
  const int64_t n_frames = chunk_frames * (n_vec * nc + 2 * B);
  const int64_t n_part = fused ? (int64_t)B * n_wg * (D + 1) + MD_STEP_MAX_Q : 0;
  double* buf = nullptr;
  GDML_TRY(ctx_alloc(ctx, (void**)&buf, (n_state + n_frames + n_part) * 8));
  auto drop = [&](int rc) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)ctx_free(ctx, buf);
    return rc;
  };
  double* d_mass = buf;
  double* half[2] = {d_mass + p->N, d_mass + p->N + n_half};
  int cur = 0;  // the half that holds the current state
  double* d_R = half[0];
  double* d_V = d_R + nc;
  double* d_F = d_V + nc;
  double* d_E = d_F + nc;
  double* d_Ek = d_E + B;
  int64_t* d_bad = (int64_t*)(half[1] + n_half);
  double* fp = half[1] + n_half + B;
  double* c_R = R_rec ? fp : nullptr;
  if (R_rec) fp += chunk_frames * nc;
  double* c_V = V_rec ? fp : nullptr;
  if (V_rec) fp += chunk_frames * nc;
  double* c_F = F_rec ? fp : nullptr;
  if (F_rec) fp += chunk_frames * nc;
  double* c_E = fp;
  double* c_Ek = c_E + chunk_frames * B;
  double* d_part = c_Ek + chunk_frames * B;
  unsigned* d_counter = (unsigned*)(d_part + (int64_t)B * n_wg * (D + 1));

  hipStream_t st = ctx->stream;
  DROP_HIP(hipMemcpyAsync(d_mass, p->mass, (size_t)p->N * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_R, R, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_V, V, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  md_fill_i64_kernel<<<ceil_div(B, 256), 256, 0, st>>>(d_bad, B, -1);
  if (fused) DROP_HIP(hipMemsetAsync(d_counter, 0, MD_STEP_MAX_Q * 8, st));
  // the caller's arrays are pageable: the copies above have to be through before they may change
  DROP_HIP(hipStreamSynchronize(st));

  MdConst C;
  C.B = B;
  C.n3 = n3;
  C.dt = p->dt;
  C.f_scale = p->f_scale;
  C.thermostat = p->thermostat;
  C.c1 = exp(-p->gamma * p->dt);
  C.c2 = sqrt(1.0 - C.c1 * C.c1);
  C.kT = p->kT;
  C.seed = p->seed;

  MdStepArgs S;
  memset(&S, 0, sizeof(S));
  if (fused) {
    S.M.xp = md.xp; S.M.jap = md.jap; S.M.aE = md.has_aE ? md.aE : nullptr;
    S.M.MP = MP; S.M.D = D; S.M.N = p->N; S.M.sig = md.sig; S.M.rows_per_wave = rows;
    S.M.part = d_part; S.M.counter = d_counter; S.C = C; S.mass = d_mass; S.bad = d_bad;
    if (p->lat && p->lat_inv) {
      memcpy(S.M.L.lat, p->lat, sizeof(S.M.L.lat));
      memcpy(S.M.L.inv, p->lat_inv, sizeof(S.M.L.inv));
      S.M.L.use = 1;
    }
  }
  int KPL = 1;
  while (KPL * 64 < D) KPL <<= 1;
  // one single-launch step from the current half of the state into the other one
  auto launch_step = [&](int init, int64_t step, const MdFrame& fr) {
    const double* in = half[cur];
    double* out = half[cur ^ 1];
    S.init = init; S.step = step; S.fr = fr;
    S.inR = in; S.inV = in + nc; S.inF = in + 2 * nc;
    S.outR = out; S.outV = out + nc; S.outF = out + 2 * nc; S.outE = out + 3 * nc; S.outEk = out + 3 * nc + B;
    const dim3 grid((unsigned)n_wg, (unsigned)B);
    switch (KPL) {
      case 1: hipLaunchKernelGGL(md_step_kernel<1>, grid, dim3(256), 0, st, S); break;
      case 2: hipLaunchKernelGGL(md_step_kernel<2>, grid, dim3(256), 0, st, S); break;
      default: hipLaunchKernelGGL(md_step_kernel<4>, grid, dim3(256), 0, st, S); break;
    }
    cur ^= 1;
  };

  // forces of the start geometry (a continued run recomputes them from R_end by the same arithmetic: the same bits as the run
  // it continues)
  if (n_steps > 0) {
    if (fused) {
      launch_step(1, p->step0, MdFrame{});
    } else {
      ctx->phase_pending.clear();
      DROP_TRY(gdml_predict_dev(ctx, d_R, B, p->lat, p->lat_inv, d_E, d_F));
    }
  }

  std::vector<int64_t> h_bad((size_t)B);
  const int pre_grid = ceil_div(nc, 256);
  int64_t t = 0, frames_done = 0;
  while (t < n_steps) {
    int64_t in_chunk = 0, steps = 0;
    while (t < n_steps && steps < MD_CHUNK_STEPS && (chunk_frames == 0 || in_chunk < chunk_frames)) {
      const int64_t step = p->step0 + t;
      if (!fused) {
        md_pre_kernel<<<pre_grid, 256, 0, st>>>(C, d_mass, d_R, d_V, d_F, d_bad, step);
        // the timer of the previous step's prediction is dropped unread: reading it would wait for that step on the host
        ctx->phase_pending.clear();
        DROP_TRY(gdml_predict_dev(ctx, d_R, B, p->lat, p->lat_inv, d_E, d_F));
      }
      ++t;
      ++steps;
      MdFrame fr = {};
      if (t % record_every == 0) {
        fr.on = 1;
        fr.R = c_R ? c_R + in_chunk * nc : nullptr;
        fr.V = c_V ? c_V + in_chunk * nc : nullptr;
        fr.F = c_F ? c_F + in_chunk * nc : nullptr;
        fr.E = c_E + in_chunk * B;
        fr.Ekin = c_Ek + in_chunk * B;
        ++in_chunk;
      }
      if (fused)
        launch_step(0, step, fr);
      else
        md_post_kernel<<<(unsigned)B, 256, 0, st>>>(C, d_mass, d_R, d_V, d_F, d_E, d_Ek, d_bad, step, fr);
    }
    DROP_HIP(hipGetLastError());
    if (in_chunk > 0) {
      const int64_t f0 = frames_done;
      if (R_rec) DROP_HIP(hipMemcpyAsync(R_rec + f0 * nc, c_R, (size_t)(in_chunk * nc) * 8, hipMemcpyDeviceToHost, st));
      if (V_rec) DROP_HIP(hipMemcpyAsync(V_rec + f0 * nc, c_V, (size_t)(in_chunk * nc) * 8, hipMemcpyDeviceToHost, st));
      if (F_rec) DROP_HIP(hipMemcpyAsync(F_rec + f0 * nc, c_F, (size_t)(in_chunk * nc) * 8, hipMemcpyDeviceToHost, st));
      if (E_rec) DROP_HIP(hipMemcpyAsync(E_rec + f0 * B, c_E, (size_t)(in_chunk * B) * 8, hipMemcpyDeviceToHost, st));
      if (Ekin_rec) DROP_HIP(hipMemcpyAsync(Ekin_rec + f0 * B, c_Ek, (size_t)(in_chunk * B) * 8, hipMemcpyDeviceToHost, st));
      frames_done += in_chunk;
    }
    DROP_HIP(hipMemcpyAsync(h_bad.data(), d_bad, (size_t)B * 8, hipMemcpyDeviceToHost, st));
    DROP_HIP(hipStreamSynchronize(st));
    bool any_bad = false;
    for (int64_t b = 0; b < B; ++b) any_bad |= h_bad[(size_t)b] >= 0;
    if (any_bad) break;  // the caller reads first_bad_step; frames up to this chunk are written
  }
  DROP_HIP(hipMemcpyAsync(R, half[cur], (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(V, half[cur] + nc, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipStreamSynchronize(st));
  if (first_bad_step && n_steps > 0) memcpy(first_bad_step, h_bad.data(), (size_t)B * 8);
  return drop(GDML_OK);
}

extern "C" int gdml_md_noise(uint64_t seed, int64_t step, int64_t B, int n3, double* xi_out, gdml_ctx* ctx) {
  if (step < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_noise: step < 0");
  if (B < 0 || B > 0x7fffffffLL || n3 < 1) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_noise: B or n3 out of range");
  if (!xi_out) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_noise: xi_out is NULL");
  if (!ctx) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_noise: ctx is NULL");
  if (B == 0) return GDML_OK;
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int64_t n = B * n3;
  double* d = nullptr;
  GDML_TRY(ctx_alloc(ctx, (void**)&d, n * 8));
  auto drop = [&](int rc) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)ctx_free(ctx, d);
    return rc;
  };
  md_noise_kernel<<<ceil_div(n, 256), 256, 0, ctx->stream>>>(seed, (uint64_t)step, B, n3, d);
  DROP_HIP(hipGetLastError());
  DROP_HIP(hipMemcpyAsync(xi_out, d, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  DROP_HIP(hipStreamSynchronize(ctx->stream));
  return drop(GDML_OK);
}

// ------------------------------------------------------------------------------------------
// Path-integral MD (gdml_pimd_run, gdml_pimd_modes; include/gdml_hip.h has the equations): B rings of P beads, state
// (B, P, 3N).  The general route's shape -- three pieces per step, stream order the only dependency:
//   pimd_pre_kernel   half kick of every bead, orthonormal real DFT over the bead index, exact free ring-polymer flow (PILE-L:
//                     half flow, Ornstein-Uhlenbeck step in mode space, half flow), transform back
//   gdml_predict_dev  on all B P geometries as one batch
//   pimd_post_kernel  second half kick, centroid, the five ring quantities by fixed trees, frame write on a recording step
// Rings always take this route (a single-launch ring step does not exist).
// ------------------------------------------------------------------------------------------
#define PIMD_MAX_BEADS 128

struct PimdConst {
  int64_t B;
  int n3, P;
  double dt, f_scale, kT;
  double wp2;  // omega_P^2
  double pkT;  // P kT, the bead temperature
  int thermostat;
  uint64_t seed;
};

// mode table (5, P): the flow over tau (dt, or dt / 2 with the thermostat) and the Ornstein-Uhlenbeck coefficients of mode k
//   [0] cos(w tau)   [1] sin(w tau) / w (tau for w = 0)   [2] -w sin(w tau)   [3] c1   [4] c2
__device__ __forceinline__ void pimd_flow(const double* __restrict__ coef, int P, int k, double& q, double& v) {
  const double cs = coef[k], sn = coef[P + k], ws = coef[2 * P + k];
  const double q1 = cs * q + sn * v;
  v = ws * q + cs * v;
  q = q1;
}

// grid = (rings, coordinate tiles); a workgroup of T threads owns all P beads of W coordinates of one ring.  Thread t works on
// coordinate t % W of the tile and on the beads (then modes, then beads again) t / W, t / W + T / W, ...  LDS: bead-space q, v
// and mode-space q, v as [bead or mode][coordinate], the coordinate contiguous: 32 P W bytes.  Every sum runs over the bead
// (mode) index in order, so the result of a coordinate depends neither on W nor on T.  Cm (P,P) is C[j][k] row-major, Ct its
// transpose.  At W = 64 a wavefront works on one mode (bead) at a time: its row of the table is wave-uniform and comes
// through scalar loads.
template <int W, int T>
__global__ void __launch_bounds__(T) pimd_pre_kernel(PimdConst C, const double* __restrict__ mass, const double* __restrict__ Cm,
                                                     const double* __restrict__ Ct, const double* __restrict__ coef,
                                                     double* __restrict__ R, double* __restrict__ V,
                                                     const double* __restrict__ F, int64_t* __restrict__ bad, int64_t step) {
  extern __shared__ __attribute__((aligned(16))) double pimd_lds[];
  constexpr int NG = T / W;
  const int P = C.P;
  double* const s_q = pimd_lds;
  double* const s_v = s_q + P * W;
  double* const s_qm = s_v + P * W;
  double* const s_vm = s_qm + P * W;
  const int cl = threadIdx.x % W;
  const int g = W == 64 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x / W)) : (int)(threadIdx.x / W);
  const int64_t b = blockIdx.x;
  const int c = (int)blockIdx.y * W + cl;  // GLOBAL coordinate: its atom is c / 3
  const bool valid = c < C.n3;
  const double m = valid ? mass[c / 3] : 1.0;
  const int64_t o = b * P * (int64_t)C.n3 + c;

  for (int j = g; j < P; j += NG) {  // half kick
    double r = 0.0, v = 0.0;
    if (valid) {
      const int64_t i = o + (int64_t)j * C.n3;
      r = R[i];
      v = V[i] + 0.5 * C.dt * (C.f_scale * F[i] / m);
    }
    s_q[j * W + cl] = r;
    s_v[j * W + cl] = v;
  }
  __syncthreads();
  const double sm = sqrt(C.pkT / m);
  for (int k = g; k < P; k += NG) {  // to modes, flow, thermostat, flow
    const double* ct = Ct + (int64_t)k * P;
    // the columns of the internal modes sum to zero, so they are applied to r_j - r_0: no cancellation against |r|, and a
    // collapsed ring has internal modes that are exactly zero
    const double oq = k ? s_q[cl] : 0.0, ov = k ? s_v[cl] : 0.0;
    double q = 0.0, v = 0.0;
    for (int j = 0; j < P; ++j) {
      const double cjk = ct[j];
      q += cjk * (s_q[j * W + cl] - oq);
      v += cjk * (s_v[j * W + cl] - ov);
    }
    pimd_flow(coef, P, k, q, v);
    if (C.thermostat) {
      const double xi = valid ? md_normal(C.seed, (uint64_t)step, (uint32_t)(b * P + k), c) : 0.0;
      v = coef[3 * P + k] * v + coef[4 * P + k] * sm * xi;
      pimd_flow(coef, P, k, q, v);
    }
    s_qm[k * W + cl] = q;
    s_vm[k * W + cl] = v;
  }
  __syncthreads();
  int nf = 0;
  for (int j = g; j < P; j += NG) {  // back to beads
    const double* cj = Cm + (int64_t)j * P;
    double r = 0.0, v = 0.0;
    for (int k = 0; k < P; ++k) {
      const double cjk = cj[k];
      r += cjk * s_qm[k * W + cl];
      v += cjk * s_vm[k * W + cl];
    }
    if (valid) {
      const int64_t i = o + (int64_t)j * C.n3;
      R[i] = r;
      V[i] = v;
      nf |= !(isfinite(r) && isfinite(v));
    }
  }
  // every thread of a ring that finds the flag unset writes the same value: no ordering needed
  if (nf && bad[b] < 0) bad[b] = step;
}

struct PimdFrame {
  double *R, *V, *F, *E, *Rc, *ring;  // slot of the frame to write in the chunk buffers (null: not recorded)
  int on;
};

// one workgroup per ring.  Thread t works on the coordinates t % 64, t % 64 + 64, ... and on the beads t / 64, t / 64 + 4, ...:
// centroid (every thread sums all beads of its coordinate in index order), second half kick, and the per-thread partial sums of
// E_kin, E_spring and sum_j (r_j - r_c) F'_j in that fixed order, then the 256-slot tree of md_post_kernel for each
__global__ void __launch_bounds__(256) pimd_post_kernel(PimdConst C, const double* __restrict__ mass, const double* __restrict__ R,
                                                        double* __restrict__ V, const double* __restrict__ F,
                                                        const double* __restrict__ E, int64_t* __restrict__ bad, int64_t step,
                                                        PimdFrame fr) {
  __shared__ double red[3][256];
  __shared__ int nonfinite;
  const int64_t b = blockIdx.x;
  const int P = C.P, n3 = C.n3;
  const int64_t o = b * P * (int64_t)n3;
  const int t = threadIdx.x, cl = t & 63, g = t >> 6;
  if (t == 0) nonfinite = 0;
  __syncthreads();
  double ek = 0.0, es = 0.0, cv = 0.0;
  int nf = 0;
  for (int c = cl; c < n3; c += 64) {
    const double m = mass[c / 3];
    double rc = 0.0;
    for (int j = 0; j < P; ++j) rc += R[o + (int64_t)j * n3 + c];
    rc = rc / (double)P;
    if (g == 0 && fr.on && fr.Rc) fr.Rc[b * n3 + c] = rc;
    for (int j = g; j < P; j += 4) {
      const int64_t i = o + (int64_t)j * n3 + c;
      const double r = R[i];
      const double rn = R[o + (int64_t)(j + 1 < P ? j + 1 : 0) * n3 + c];
      const double f = F[i];
      const double v = V[i] + 0.5 * C.dt * (C.f_scale * f / m);
      V[i] = v;
      const double d = r - rn;
      ek += 0.5 * m * v * v;
      es += 0.5 * m * C.wp2 * d * d;
      cv += (r - rc) * f;
      nf |= !(isfinite(v) && isfinite(f));
      if (fr.on) {
        if (fr.R) fr.R[i] = r;
        if (fr.V) fr.V[i] = v;
        if (fr.F) fr.F[i] = f;
      }
    }
  }
  red[0][t] = ek;
  red[1][t] = es;
  red[2][t] = cv;
  if (nf) nonfinite = 1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      red[0][t] += red[0][t + s];
      red[1][t] += red[1][t + s];
      red[2][t] += red[2][t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    double ep = 0.0;
    for (int j = 0; j < P; ++j) {
      const double e = E[b * P + j];
      ep += e;
      if (fr.on && fr.E) fr.E[b * P + j] = e;
    }
    // a velocity may be finite while its square is not: the ring's sums are part of the check
    if ((nonfinite || !isfinite(ep) || !isfinite(red[0][0] + red[1][0] + red[2][0])) && bad[b] < 0) bad[b] = step;
    if (fr.on) {
      double* q = fr.ring + b * 5;
      q[0] = ep / (double)P;
      q[1] = red[0][0];
      q[2] = red[1][0];
      q[3] = 0.5 * (double)n3 * C.kT - C.f_scale / (2.0 * (double)P) * red[2][0];
      q[4] = 0.5 * (double)n3 * (double)P * C.kT - red[1][0] / (double)P;
    }
  }
}

// C[j][k] (row j, column k) of the orthonormal real DFT over the bead index and the mode frequencies, fp64 on the host.  The
// angle is reduced exactly first: 2 pi (j k mod P) / P.
static void pimd_mode_tables(int P, double kT, double hbar, double* Cm, double* omega) {
  const double pi = 3.14159265358979323846;
  const double wP = (double)P * kT / hbar;
  for (int k = 0; k < P; ++k) omega[k] = 2.0 * wP * sin((double)k * pi / (double)P);
  for (int j = 0; j < P; ++j)
    for (int k = 0; k < P; ++k) {
      const double ang = 2.0 * pi * (double)((j * k) % P) / (double)P;
      double v;
      if (k == 0) v = 1.0 / sqrt((double)P);
      else if (2 * k < P) v = sqrt(2.0 / (double)P) * cos(ang);
      else if (2 * k == P) v = ((j & 1) ? -1.0 : 1.0) / sqrt((double)P);
      else v = sqrt(2.0 / (double)P) * sin(ang);
      Cm[j * P + k] = v;
    }
}

extern "C" int gdml_pimd_modes(int beads, double kT, double hbar, double* C, double* omega) {
  if (beads < 1 || beads > PIMD_MAX_BEADS) return gdml_fail(nullptr, GDML_ERR_INVALID, "gdml_pimd_modes: beads outside 1..128");
  if (!(hbar > 0.0) || !isfinite(hbar)) return gdml_fail(nullptr, GDML_ERR_INVALID, "gdml_pimd_modes: hbar must be positive and finite");
  if (!(kT >= 0.0) || !isfinite(kT)) return gdml_fail(nullptr, GDML_ERR_INVALID, "gdml_pimd_modes: kT < 0");
  if (!C || !omega) return gdml_fail(nullptr, GDML_ERR_INVALID, "gdml_pimd_modes: C or omega is NULL");
  pimd_mode_tables(beads, kT, hbar, C, omega);
  return GDML_OK;
}

// argument checks; ctx may be NULL (the message then goes where gdml_ctx_create's goes)
static int pimd_check(gdml_ctx* ctx, const gdml_pimd_params* p, const double* R, const double* V, int64_t n_steps,
                      int64_t record_every) {
  if (!p) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: params is NULL");
  if (n_steps < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: n_steps < 0");
  if (record_every < 1) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: record_every < 1");
  if (p->B < 0 || p->B > 0x7fffffffLL) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: B out of range");
  if (p->N < 1 || p->N > GDML_MAX_ATOMS) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: N out of range");
  if (p->beads < 1 || p->beads > PIMD_MAX_BEADS) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: beads outside 1..128");
  if (p->B * p->beads > 0x7fffffffLL) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: B * beads must stay below 2^31");
  if (!(p->dt > 0.0) || !isfinite(p->dt)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: dt must be positive and finite");
  if (!isfinite(p->f_scale)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: f_scale is not finite");
  if (!p->mass) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: mass is NULL");
  for (int a = 0; a < p->N; ++a)
    if (!(p->mass[a] > 0.0) || !isfinite(p->mass[a]))
      return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: mass of atom %d must be positive and finite", a);
  if ((p->lat == nullptr) != (p->lat_inv == nullptr))
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: lattice and inverse must both be given or both NULL");
  if (p->thermostat != 0 && p->thermostat != 1)
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: thermostat must be 0 (none) or 1 (PILE-L)");
  if (!(p->gamma_centroid >= 0.0) || !isfinite(p->gamma_centroid))
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: gamma_centroid < 0");
  if (!(p->pile_lambda > 0.0) || !isfinite(p->pile_lambda))
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: pile_lambda must be positive and finite");
  if (!(p->kT >= 0.0) || !isfinite(p->kT)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: kT < 0");
  if (p->beads > 1 && !(p->kT > 0.0)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: kT must be positive with more than one bead");
  if (!(p->hbar > 0.0) || !isfinite(p->hbar)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: hbar must be positive and finite");
  if (p->step0 < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: step0 < 0");
  if (!R || !V) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: R or V is NULL");
  return GDML_OK;
}

extern "C" int gdml_pimd_run(gdml_ctx* ctx, const gdml_pimd_params* p, double* R, double* V, int64_t n_steps, int64_t record_every,
                             double* R_rec, double* V_rec, double* F_rec, double* E_rec, double* Rc_rec, double* ring_rec,
                             int64_t* first_bad_step) {
  GDML_TRY(pimd_check(ctx, p, R, V, n_steps, record_every));
  if (!ctx) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: ctx is NULL");
  Model& md = ctx->model;
  if (!md.xp) return gdml_fail(ctx, GDML_ERR_STATE, "gdml_pimd_run: upload a model first");
  if (md.N != p->N) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: N = %d but the model has %d atoms", p->N, md.N);
  const int64_t B = p->B;
  const int P = p->beads, n3 = 3 * p->N;
  if (first_bad_step)
    for (int64_t b = 0; b < B; ++b) first_bad_step[b] = -1;
  if (B == 0) return GDML_OK;
  HIP_CHECK(ctx, hipSetDevice(ctx->device));

  // tile width of pimd_pre_kernel: 64 coordinates where its LDS (32 P W bytes) stays within 128 KiB, else 32; option
  // predict.pimd_tile (32 or 64) asks for one of them where it fits
  int W = P <= 64 ? 64 : 32;
  const int w_opt = ctx_opt_i(ctx, "predict.pimd_tile", 0);
  if (w_opt == 32) W = 32;
  const size_t pre_lds = (size_t)32 * P * W;
  // 1024 threads beyond 16 beads: a thread then carries at most 128 W / 1024 modes
  const int T = P > 16 ? 1024 : 256;
  using PreFn = void (*)(PimdConst, const double*, const double*, const double*, const double*, double*, double*, const double*,
                         int64_t*, int64_t);
  const PreFn pre = W == 64 ? (T == 1024 ? (PreFn)pimd_pre_kernel<64, 1024> : (PreFn)pimd_pre_kernel<64, 256>)
                            : (T == 1024 ? (PreFn)pimd_pre_kernel<32, 1024> : (PreFn)pimd_pre_kernel<32, 256>);
  const dim3 pre_grid((unsigned)B, (unsigned)ceil_div(n3, W));

  const int64_t BP = B * P;
  const int64_t nc = BP * n3;
  const int64_t n_rec = n_steps / record_every;
  const int n_vec = (R_rec ? 1 : 0) + (V_rec ? 1 : 0) + (F_rec ? 1 : 0);
  const int64_t frame_len = n_vec * nc + (E_rec ? BP : 0) + (Rc_rec ? B * n3 : 0) + 5 * B;
  int64_t chunk_frames = MD_CHUNK_BYTES / (frame_len * 8);
  const int64_t opt = (int64_t)ctx_opt(ctx, "predict.md_chunk_frames", 0.0);
  if (opt > 0 && opt < chunk_frames) chunk_frames = opt;
  if (chunk_frames < 1) chunk_frames = 1;
  if (chunk_frames > n_rec) chunk_frames = n_rec;  // 0: nothing is recorded (n_steps < record_every)

  // one allocation: mass | C | C^T | mode table | R | V | F | E | bad | frames of a chunk (R, V, F, E, Rc as requested, ring)
  const int64_t n_tab = p->N + 2 * (int64_t)P * P + 5 * P;
  const int64_t n_state = n_tab + 3 * nc + BP + B;
  double* buf = nullptr;
  GDML_TRY(ctx_alloc(ctx, (void**)&buf, (n_state + chunk_frames * frame_len) * 8));
  auto drop = [&](int rc) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)ctx_free(ctx, buf);
    return rc;
  };
  double* d_mass = buf;
  double* d_Cm = d_mass + p->N;
  double* d_Ct = d_Cm + (int64_t)P * P;
  double* d_coef = d_Ct + (int64_t)P * P;
  double* d_R = d_coef + 5 * P;
  double* d_V = d_R + nc;
  double* d_F = d_V + nc;
  double* d_E = d_F + nc;
  int64_t* d_bad = (int64_t*)(d_E + BP);
  double* fp = d_E + BP + B;
  double* c_R = R_rec ? fp : nullptr;
  if (R_rec) fp += chunk_frames * nc;
  double* c_V = V_rec ? fp : nullptr;
  if (V_rec) fp += chunk_frames * nc;
  double* c_F = F_rec ? fp : nullptr;
  if (F_rec) fp += chunk_frames * nc;
  double* c_E = E_rec ? fp : nullptr;
  if (E_rec) fp += chunk_frames * BP;
  double* c_Rc = Rc_rec ? fp : nullptr;
  if (Rc_rec) fp += chunk_frames * B * n3;
  double* c_ring = fp;

  // host tables: the transform, its transpose, and per mode the flow over tau and the thermostat's coefficients
  const double wP = (double)P * p->kT / p->hbar;
  const double tau = p->thermostat ? 0.5 * p->dt : p->dt;
  std::vector<double> h_tab((size_t)(2 * P * P + 5 * P)), h_w((size_t)P);
  double* h_Cm = h_tab.data();
  double* h_Ct = h_Cm + P * P;
  double* h_coef = h_Ct + P * P;
  pimd_mode_tables(P, p->kT, p->hbar, h_Cm, h_w.data());
  for (int j = 0; j < P; ++j)
    for (int k = 0; k < P; ++k) h_Ct[k * P + j] = h_Cm[j * P + k];
  for (int k = 0; k < P; ++k) {
    const double w = h_w[(size_t)k];
    h_coef[k] = cos(w * tau);
    h_coef[P + k] = w > 0.0 ? sin(w * tau) / w : tau;
    h_coef[2 * P + k] = -w * sin(w * tau);
    const double c1 = exp(-(k == 0 ? p->gamma_centroid : p->pile_lambda * 2.0 * w) * p->dt);
    h_coef[3 * P + k] = c1;
    h_coef[4 * P + k] = sqrt(1.0 - c1 * c1);
  }

  hipStream_t st = ctx->stream;
  DROP_HIP(hipMemcpyAsync(d_mass, p->mass, (size_t)p->N * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_Cm, h_tab.data(), h_tab.size() * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_R, R, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_V, V, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  md_fill_i64_kernel<<<ceil_div(B, 256), 256, 0, st>>>(d_bad, B, -1);
  // the caller's arrays are pageable: the copies above have to be through before they may change
  DROP_HIP(hipStreamSynchronize(st));
  if (pre_lds > 64 * 1024) DROP_HIP(hipFuncSetAttribute((const void*)pre, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pre_lds));

  PimdConst C;
  C.B = B;
  C.n3 = n3;
  C.P = P;
  C.dt = p->dt;
  C.f_scale = p->f_scale;
  C.kT = p->kT;
  C.wp2 = wP * wP;
  C.pkT = (double)P * p->kT;
  C.thermostat = p->thermostat;
  C.seed = p->seed;

  // forces of the start geometry (a continued run recomputes them from R_end by the same call: the same bits as the run it
  // continues)
  if (n_steps > 0) {
    ctx->phase_pending.clear();
    DROP_TRY(gdml_predict_dev(ctx, d_R, BP, p->lat, p->lat_inv, d_E, d_F));
  }

  std::vector<int64_t> h_bad((size_t)B);
  int64_t t = 0, frames_done = 0;
  while (t < n_steps) {
    int64_t in_chunk = 0, steps = 0;
    while (t < n_steps && steps < MD_CHUNK_STEPS && (chunk_frames == 0 || in_chunk < chunk_frames)) {
      const int64_t step = p->step0 + t;
      pre<<<pre_grid, T, pre_lds, st>>>(C, d_mass, d_Cm, d_Ct, d_coef, d_R, d_V, d_F, d_bad, step);
      // the timer of the previous step's prediction is dropped unread: reading it would wait for that step on the host
      ctx->phase_pending.clear();
      DROP_TRY(gdml_predict_dev(ctx, d_R, BP, p->lat, p->lat_inv, d_E, d_F));
      ++t;
      ++steps;
      PimdFrame fr = {};
      if (t % record_every == 0) {
        fr.on = 1;
        fr.R = c_R ? c_R + in_chunk * nc : nullptr;
        fr.V = c_V ? c_V + in_chunk * nc : nullptr;
        fr.F = c_F ? c_F + in_chunk * nc : nullptr;
        fr.E = c_E ? c_E + in_chunk * BP : nullptr;
        fr.Rc = c_Rc ? c_Rc + in_chunk * B * n3 : nullptr;
        fr.ring = c_ring + in_chunk * B * 5;
        ++in_chunk;
      }
      pimd_post_kernel<<<(unsigned)B, 256, 0, st>>>(C, d_mass, d_R, d_V, d_F, d_E, d_bad, step, fr);
    }
    DROP_HIP(hipGetLastError());
    if (in_chunk > 0) {
      const int64_t f0 = frames_done;
      if (R_rec) DROP_HIP(hipMemcpyAsync(R_rec + f0 * nc, c_R, (size_t)(in_chunk * nc) * 8, hipMemcpyDeviceToHost, st));
      if (V_rec) DROP_HIP(hipMemcpyAsync(V_rec + f0 * nc, c_V, (size_t)(in_chunk * nc) * 8, hipMemcpyDeviceToHost, st));
      if (F_rec) DROP_HIP(hipMemcpyAsync(F_rec + f0 * nc, c_F, (size_t)(in_chunk * nc) * 8, hipMemcpyDeviceToHost, st));
      if (E_rec) DROP_HIP(hipMemcpyAsync(E_rec + f0 * BP, c_E, (size_t)(in_chunk * BP) * 8, hipMemcpyDeviceToHost, st));
      if (Rc_rec)
        DROP_HIP(hipMemcpyAsync(Rc_rec + f0 * B * n3, c_Rc, (size_t)(in_chunk * B * n3) * 8, hipMemcpyDeviceToHost, st));
      if (ring_rec)
        DROP_HIP(hipMemcpyAsync(ring_rec + f0 * B * 5, c_ring, (size_t)(in_chunk * B * 5) * 8, hipMemcpyDeviceToHost, st));
      frames_done += in_chunk;
    }
    DROP_HIP(hipMemcpyAsync(h_bad.data(), d_bad, (size_t)B * 8, hipMemcpyDeviceToHost, st));
    DROP_HIP(hipStreamSynchronize(st));
    bool any_bad = false;
    for (int64_t b = 0; b < B; ++b) any_bad |= h_bad[(size_t)b] >= 0;
    if (any_bad) break;  // the caller reads first_bad_step; frames up to this chunk are written
  }
  DROP_HIP(hipMemcpyAsync(R, d_R, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(V, d_V, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipStreamSynchronize(st));
  if (first_bad_step && n_steps > 0) memcpy(first_bad_step, h_bad.data(), (size_t)B * 8);
  return drop(GDML_OK);
}

// ------------------------------------------------------------------------------------------
// Geometry relaxation (gdml_relax_run): B independent geometries descend by FIRE (Bitzek et al., Phys. Rev. Lett. 97, 170201
// (2006)) in the form ASE's FIRE uses -- unit masses, the whole 3N-vector step clipped.  The step (the contract;
// include/gdml_hip.h and tests/_relax_ref.py state the same):
//   g = f_scale F'; sums and norms over a replica's 3N coordinates; state v, dt, alpha, n_pos, n_taken per replica.
//   Evaluation t = 0, 1, ... of an active replica:
//   1. E', F' = predictor(r);  f_atom = max over atoms |g_atom|;  both into the history; non-finite r, v, F', E' -> bad[q] = t
//   2. f_atom < fmax: converged -- r, v, dt, alpha, n_pos, n_taken, E', F' freeze, never written again
//   3. else t = max_steps: stops unconverged, freezes the same way
//   4. else, if n_taken > 0:  p = g . v;
//        p > 0:   v <- (1 - alpha) v + (alpha |v| / |g|) g;  if n_pos > n_min: dt <- min(dt f_inc, dt_max), alpha <- alpha f_alpha;
//                 n_pos += 1
//        p <= 0:  v <- 0, alpha <- alpha_start, dt <- dt f_dec, n_pos <- 0
//      v <- v + dt g;  Delta = dt v;  |Delta| > max_step: Delta <- Delta (max_step / |Delta|);  r <- r + Delta;  n_taken += 1
// Sums: per-thread partial sums in index order, then the 256-slot tree of md_post_kernel.  Two routes, ONE update function
// (relax_finish) on both:
//   general:       gdml_predict_dev for all B geometries into scratch (frozen replicas' results are discarded), then
//                  relax_update_kernel, one workgroup per replica
//   single launch: relax_step_kernel (D <= 256, B <= 8), the predictor's share being md_step_kernel's (step_partials,
//                  step_gather, step_force); r(t+1) into the other half of a ping-pong buffer
// The host synchronises once per chunk and reads the status words; it stops when no replica is active.
// ------------------------------------------------------------------------------------------
struct RelaxConst {
  int n3;
  double f_scale, fmax, dt_max, max_step, f_inc, f_dec, alpha_start, f_alpha;
  int64_t n_min;
};
struct RelaxState {  // per-replica state in device memory
  double *V, *F, *E, *dt, *alpha;
  int64_t *n_pos, *n_taken;
  int64_t* status;  // (B,2): [0] -1 active, 0 budget used up, 1 converged; [1] the evaluation at which it froze
  int64_t* bad;
};
struct RelaxSlot {  // where this evaluation goes in the chunk buffers
  double *E, *fat;  // (B) rows of the history
  double* R;        // (B,3N) frame; null when this is no recording evaluation
};

// Steps 1-4 for replica q once its F' is known, called by all 256 threads of one workgroup.  r: positions of this evaluation,
// fp: F', e: E'; r_next: where r(t+1) goes (may be r itself: every coordinate is read and written by one thread); r_keep: where
// a freezing replica's r is written as well (null: nowhere).  red: 4 x 256 doubles of LDS.
__device__ __forceinline__ void relax_finish(const RelaxConst& C, const RelaxState& S, const RelaxSlot& sl, int64_t q, int64_t t,
                                             int last, const double* r, const double* fp, double e, double* r_next,
                                             double* r_keep, double (&red)[4][256]) {
  const int tid = threadIdx.x, n3 = C.n3;
  const int64_t o = q * n3;
  double dt = S.dt[q], alpha = S.alpha[q];
  int64_t n_pos = S.n_pos[q];
  const int64_t n_taken = S.n_taken[q];

  double gv = 0.0, gg = 0.0, vv = 0.0, fa = 0.0;
  int nf = 0;
  for (int k = tid; k < n3; k += 256) {
    const double f = fp[k], v = S.V[o + k], g = C.f_scale * f;
    gv += g * v;
    gg += g * g;
    vv += v * v;
    nf |= !(isfinite(r[k]) && isfinite(v) && isfinite(f));
    S.F[o + k] = f;
    if (sl.R) sl.R[o + k] = r[k];
  }
  for (int a = tid; 3 * a < n3; a += 256) {
    const double g0 = C.f_scale * fp[3 * a], g1 = C.f_scale * fp[3 * a + 1], g2 = C.f_scale * fp[3 * a + 2];
    const double nrm = sqrt(g0 * g0 + g1 * g1 + g2 * g2);
    fa = nrm > fa ? nrm : fa;
  }
  red[0][tid] = gv;
  red[1][tid] = gg;
  red[2][tid] = vv;
  red[3][tid] = fa;
  nf = __syncthreads_or(nf);
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
      red[2][tid] += red[2][tid + s];
      red[3][tid] = red[3][tid + s] > red[3][tid] ? red[3][tid + s] : red[3][tid];
    }
    __syncthreads();
  }
  const double p = red[0][0], g_nrm = sqrt(red[1][0]), v_nrm = sqrt(red[2][0]), f_atom = red[3][0];
  const bool bad_now = nf || !isfinite(e);
  const bool conv = !bad_now && f_atom < C.fmax;  // (the maximum skips a NaN)
  if (tid == 0) {
    S.E[q] = e;
    sl.E[q] = e;
    sl.fat[q] = f_atom;
    if (bad_now && S.bad[q] < 0) S.bad[q] = t;
  }
  if (conv || last) {  // frozen from here on: no later launch writes anything of this replica
    if (r_keep)
      for (int k = tid; k < n3; k += 256) r_keep[k] = r[k];
    if (tid == 0) {
      S.status[2 * q] = conv ? 1 : 0;
      S.status[2 * q + 1] = t;
    }
    return;
  }

  int mode = 0;  // 0: v as it is (the first step of a lifetime), 1: mixed with the force direction, 2: zeroed
  double cv = 1.0, cg = 0.0;
  if (n_taken > 0) {
    if (p > 0.0) {
      mode = 1;
      cv = 1.0 - alpha;
      cg = alpha * v_nrm / g_nrm;
      if (n_pos > C.n_min) {
        dt = fmin(dt * C.f_inc, C.dt_max);
        alpha = alpha * C.f_alpha;
      }
      n_pos += 1;
    } else {
      mode = 2;
      alpha = C.alpha_start;
      dt = dt * C.f_dec;
      n_pos = 0;
    }
  }
  double dd = 0.0;
  for (int k = tid; k < n3; k += 256) {
    const double g = C.f_scale * fp[k];
    double v = S.V[o + k];
    if (mode == 1) v = cv * v + cg * g;
    if (mode == 2) v = 0.0;
    v = v + dt * g;
    S.V[o + k] = v;
    const double d = dt * v;
    dd += d * d;
  }
  __syncthreads();  // every thread has read the first tree's results
  red[0][tid] = dd;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[0][tid] += red[0][tid + s];
    __syncthreads();
  }
  const double d_nrm = sqrt(red[0][0]);
  const bool clip = d_nrm > C.max_step;
  const double scale = C.max_step / d_nrm;
  for (int k = tid; k < n3; k += 256) {
    double d = dt * S.V[o + k];
    if (clip) d = d * scale;
    r_next[k] = r[k] + d;
  }
  if (tid == 0) {
    S.dt[q] = dt;
    S.alpha[q] = alpha;
    S.n_pos[q] = n_pos;
    S.n_taken[q] = n_taken + 1;
  }
}

// general route, one workgroup per replica: F', E' of all B geometries lie in Ft, Et (gdml_predict_dev); a frozen replica's
// are ignored
__global__ void __launch_bounds__(256) relax_update_kernel(RelaxConst C, RelaxState S, RelaxSlot sl, double* R, const double* Ft,
                                                           const double* Et, int64_t t, int last) {
  __shared__ double red[4][256];
  const int64_t q = blockIdx.x;
  if (S.status[2 * q] >= 0) return;
  double* r = R + q * C.n3;
  relax_finish(C, S, sl, q, t, last, r, Ft + q * C.n3, Et[q], r, nullptr, red);
}

struct RelaxStepArgs {
  StepModel M;
  RelaxConst C;
  RelaxState S;
  RelaxSlot sl;
  const double* inR;
  double* outR;
  int64_t t;
  int last;
};

// single-launch evaluation: grid = (row shares, replicas) as md_step_kernel's.  The workgroups of a frozen replica return at
// once (its status word was written by an earlier launch).  The replica's last workgroup back-projects F' and runs
// relax_finish with its r in LDS; r(t+1) -- or the frozen r -- goes into the other half of the ping-pong buffer.
template <int KPL>
__global__ void __launch_bounds__(256) relax_step_kernel(RelaxStepArgs A) {
  __shared__ double s_fx[4][KPL * 64];
  __shared__ double s_E[4];
  __shared__ double s_g[KPL * 64 * 3];
  __shared__ double s_r[MD_STEP_MAX_COORDS], s_f[MD_STEP_MAX_COORDS];
  __shared__ double red[4][256];
  __shared__ double s_Eq;
  __shared__ unsigned s_ticket;
  const int tid = threadIdx.x;
  const int N = A.M.N, n3 = 3 * N;
  const int q = (int)blockIdx.y;
  if (A.S.status[2 * q] >= 0) return;
  if (tid < n3) s_r[tid] = A.inR[(int64_t)q * n3 + tid];
  __syncthreads();

  if (!step_partials<KPL>(A.M, s_r, s_fx, s_E, s_ticket)) return;
  double* fxs = &s_fx[0][0];
  step_gather(A.M, s_r, fxs, s_g, s_Eq);
  if (tid < n3) s_f[tid] = step_force(N, s_g, fxs, tid);
  __syncthreads();
  double* out = A.outR + (int64_t)q * n3;
  relax_finish(A.C, A.S, A.sl, q, A.t, A.last, s_r, s_f, s_Eq, out, out, red);
  if (tid == 0) A.M.counter[q] = 0u;  // the next launch on the stream finds it reset
}

// argument checks; ctx may be NULL (the message then goes where gdml_ctx_create's goes)
static int relax_check(gdml_ctx* ctx, const gdml_relax_params* p, const double* R, const double* V, const double* dt,
                       const double* alpha, const int64_t* n_pos, const int64_t* n_taken, int64_t max_steps, int64_t record_every,
                       const double* R_rec, const double* E_hist, const double* fmax_hist, const double* E_end,
                       const double* F_end, const int64_t* status) {
  if (!p) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: params is NULL");
  if (max_steps < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: max_steps < 0");
  if (record_every < 0 || (R_rec && record_every < 1))
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: record_every < 0, or < 1 with R_rec");
  if (p->B < 0 || p->B > 0x7fffffffLL) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: B out of range");
  if (p->N < 1 || p->N > GDML_MAX_ATOMS) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: N out of range");
  if (!isfinite(p->f_scale)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: f_scale is not finite");
  if (!(p->fmax > 0.0) || !isfinite(p->fmax)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: fmax must be positive and finite");
  if (!(p->max_step > 0.0) || !isfinite(p->max_step))
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: max_step must be positive and finite");
  if (!(p->f_inc >= 1.0) || !isfinite(p->f_inc)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: f_inc < 1");
  if (!(p->f_dec > 0.0 && p->f_dec < 1.0)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: f_dec outside (0, 1)");
  if (!(p->alpha_start > 0.0 && p->alpha_start <= 1.0))
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: alpha_start outside (0, 1]");
  if (!(p->f_alpha > 0.0 && p->f_alpha <= 1.0)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: f_alpha outside (0, 1]");
  if (p->n_min < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: n_min < 0");
  if ((p->lat == nullptr) != (p->lat_inv == nullptr))
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: lattice and inverse must both be given or both NULL");
  if (!R || !V || !dt || !alpha || !n_pos || !n_taken)
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: a state array (R, V, dt, alpha, n_pos, n_taken) is NULL");
  if (!E_hist || !fmax_hist || !E_end || !F_end || !status)
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: an output array (E_hist, fmax_hist, E_end, F_end, status) is NULL");
  if (!(p->dt_max > 0.0) || !isfinite(p->dt_max))
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: dt_max must be positive and finite");
  for (int64_t b = 0; b < p->B; ++b) {
    if (!(dt[b] > 0.0) || !isfinite(dt[b]))
      return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: dt of replica %lld must be positive and finite", (long long)b);
    if (p->dt_max < dt[b])
      return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: dt_max is below dt of replica %lld", (long long)b);
  }
  return GDML_OK;
}

extern "C" int gdml_relax_run(gdml_ctx* ctx, const gdml_relax_params* p, double* R, double* V, double* dt, double* alpha,
                              int64_t* n_pos, int64_t* n_taken, int64_t max_steps, int64_t record_every, double* R_rec,
                              double* E_hist, double* fmax_hist, double* E_end, double* F_end, int64_t* status,
                              int64_t* first_bad_step) {
  GDML_TRY(relax_check(ctx, p, R, V, dt, alpha, n_pos, n_taken, max_steps, record_every, R_rec, E_hist, fmax_hist, E_end, F_end,
                       status));
  if (!ctx) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: ctx is NULL");
  Model& md = ctx->model;
  if (!md.xp) return gdml_fail(ctx, GDML_ERR_STATE, "gdml_relax_run: upload a model first");
  if (md.N != p->N) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: N = %d but the model has %d atoms", p->N, md.N);
  const int64_t B = p->B;
  const int n3 = 3 * p->N;
  if (first_bad_step)
    for (int64_t b = 0; b < B; ++b) first_bad_step[b] = -1;
  if (B == 0) return GDML_OK;
  HIP_CHECK(ctx, hipSetDevice(ctx->device));

  const int64_t nc = B * n3;
  const int64_t n_eval_max = max_steps + 1;
  // evaluations per chunk, and frames of R per chunk where they are recorded
  int64_t chunk_steps = (int64_t)ctx_opt(ctx, "predict.relax_chunk_steps", 32.0);
  if (chunk_steps < 1) chunk_steps = 1;
  if (chunk_steps > n_eval_max) chunk_steps = n_eval_max;
  int64_t chunk_frames = 0;
  if (R_rec) {
    chunk_frames = MD_CHUNK_BYTES / (nc * 8);
    const int64_t opt = (int64_t)ctx_opt(ctx, "predict.md_chunk_frames", 0.0);
    if (opt > 0 && opt < chunk_frames) chunk_frames = opt;
    if (chunk_frames < 1) chunk_frames = 1;
    if (chunk_frames > chunk_steps) chunk_frames = chunk_steps;
  }

  const int D = md.D;
  const bool fused = B <= MD_STEP_MAX_Q && D >= 1 && D <= 256 && n3 <= MD_STEP_MAX_COORDS && !ctx->profiling &&
                     ctx_opt_i(ctx, "predict.relax_fused", 1) != 0;
  const int64_t MP = md.M * md.P;
  int rows = ctx_opt_i(ctx, "predict.fused_rows", 16);  // the row split of predict_fused: at most 4 x 256 wavefronts
  if (rows < 2) rows = 2;
  while ((MP + rows - 1) / rows > 1024) rows *= 2;
  const int n_wg = (int)(((MP + rows - 1) / rows + 3) / 4);

  // one allocation: two halves of R (the general route works in the first) | V | F | F', E' of the general route's prediction
  // | E | dt | alpha | n_pos | n_taken | status | bad | a chunk of the history (E, f_atom) and of frames | partials, tickets
  const int64_t n_state = 4 * nc + (fused ? 0 : nc + B) + 8 * B;
  const int64_t n_chunk = 2 * chunk_steps * B + chunk_frames * nc;
  const int64_t n_part = fused ? (int64_t)B * n_wg * (D + 1) + MD_STEP_MAX_Q : 0;
  double* buf = nullptr;
  GDML_TRY(ctx_alloc(ctx, (void**)&buf, (n_state + n_chunk + n_part) * 8));
  auto drop = [&](int rc) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)ctx_free(ctx, buf);
    return rc;
  };
  double* half[2] = {buf, buf + nc};
  int cur = 0;  // the half that holds the current positions
  double* d_V = buf + 2 * nc;
  double* d_F = d_V + nc;
  double* d_Ft = d_F + nc;
  double* d_Et = d_Ft + (fused ? 0 : nc);
  double* d_E = d_Et + (fused ? 0 : B);
  double* d_dt = d_E + B;
  double* d_alpha = d_dt + B;
  int64_t* d_npos = (int64_t*)(d_alpha + B);
  int64_t* d_ntaken = d_npos + B;
  int64_t* d_status = d_ntaken + B;
  int64_t* d_bad = d_status + 2 * B;
  double* c_E = (double*)(d_bad + B);
  double* c_fat = c_E + chunk_steps * B;
  double* c_R = c_fat + chunk_steps * B;
  double* d_part = c_R + chunk_frames * nc;
  unsigned* d_counter = (unsigned*)(d_part + (int64_t)B * n_wg * (D + 1));

  hipStream_t st = ctx->stream;
  DROP_HIP(hipMemcpyAsync(half[0], R, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_V, V, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_dt, dt, (size_t)B * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_alpha, alpha, (size_t)B * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_npos, n_pos, (size_t)B * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_ntaken, n_taken, (size_t)B * 8, hipMemcpyHostToDevice, st));
  md_fill_i64_kernel<<<ceil_div(3 * B, 256), 256, 0, st>>>(d_status, 3 * B, -1);  // status and bad
  if (fused) DROP_HIP(hipMemsetAsync(d_counter, 0, MD_STEP_MAX_Q * 8, st));
  // the caller's arrays are pageable: the copies above have to be through before they may change
  DROP_HIP(hipStreamSynchronize(st));

  RelaxConst C;
  C.n3 = n3;
  C.f_scale = p->f_scale;
  C.fmax = p->fmax;
  C.dt_max = p->dt_max;
  C.max_step = p->max_step;
  C.f_inc = p->f_inc;
  C.f_dec = p->f_dec;
  C.alpha_start = p->alpha_start;
  C.f_alpha = p->f_alpha;
  C.n_min = p->n_min;
  RelaxState S = {d_V, d_F, d_E, d_dt, d_alpha, d_npos, d_ntaken, d_status, d_bad};

  RelaxStepArgs A;
  memset(&A, 0, sizeof(A));
  if (fused) {
    A.M.xp = md.xp; A.M.jap = md.jap; A.M.aE = md.has_aE ? md.aE : nullptr;
    A.M.MP = MP; A.M.D = D; A.M.N = p->N; A.M.sig = md.sig; A.M.rows_per_wave = rows;
    A.M.part = d_part; A.M.counter = d_counter; A.C = C; A.S = S;
    if (p->lat && p->lat_inv) {
      memcpy(A.M.L.lat, p->lat, sizeof(A.M.L.lat));
      memcpy(A.M.L.inv, p->lat_inv, sizeof(A.M.L.inv));
      A.M.L.use = 1;
    }
  }
  int KPL = 1;
  while (KPL * 64 < D) KPL <<= 1;

  // status (B,2), bad (B) and the chunk's history lie side by side: ONE copy per chunk brings them to the host
  const int64_t n_out = 3 * B + 2 * chunk_steps * B;
  std::vector<int64_t> h_out((size_t)n_out, -1);
  const int64_t* h_flags = h_out.data();
  const double* h_E = (const double*)(h_out.data() + 3 * B);
  const double* h_fat = h_E + chunk_steps * B;
  int64_t t = 0, frames_done = 0;
  bool active = true, any_bad = false;
  while (t <= max_steps && active && !any_bad) {
    const int64_t t0 = t;
    int64_t in_chunk = 0;
    for (; t <= max_steps && t - t0 < chunk_steps; ++t) {
      const bool rec = R_rec && t % record_every == 0;
      if (rec && in_chunk == chunk_frames) break;
      RelaxSlot sl = {c_E + (t - t0) * B, c_fat + (t - t0) * B, rec ? c_R + in_chunk * nc : nullptr};
      if (rec) ++in_chunk;
      const int last = t == max_steps;
      if (fused) {
        A.sl = sl; A.t = t; A.last = last;
        A.inR = half[cur]; A.outR = half[cur ^ 1];
        const dim3 grid((unsigned)n_wg, (unsigned)B);
        switch (KPL) {
          case 1: hipLaunchKernelGGL(relax_step_kernel<1>, grid, dim3(256), 0, st, A); break;
          case 2: hipLaunchKernelGGL(relax_step_kernel<2>, grid, dim3(256), 0, st, A); break;
          default: hipLaunchKernelGGL(relax_step_kernel<4>, grid, dim3(256), 0, st, A); break;
        }
        cur ^= 1;
      } else {
        // the timer of the previous evaluation's prediction is dropped unread: reading it would wait for it on the host
        ctx->phase_pending.clear();
        DROP_TRY(gdml_predict_dev(ctx, half[0], B, p->lat, p->lat_inv, d_Et, d_Ft));
        relax_update_kernel<<<(unsigned)B, 256, 0, st>>>(C, S, sl, half[0], d_Ft, d_Et, t, last);
      }
    }
    DROP_HIP(hipGetLastError());
    if (in_chunk > 0) {
      DROP_HIP(hipMemcpyAsync(R_rec + frames_done * nc, c_R, (size_t)(in_chunk * nc) * 8, hipMemcpyDeviceToHost, st));
      frames_done += in_chunk;
    }
    DROP_HIP(hipMemcpyAsync(h_out.data(), d_status, (size_t)n_out * 8, hipMemcpyDeviceToHost, st));
    DROP_HIP(hipStreamSynchronize(st));
    memcpy(E_hist + t0 * B, h_E, (size_t)((t - t0) * B) * 8);
    memcpy(fmax_hist + t0 * B, h_fat, (size_t)((t - t0) * B) * 8);
    active = false;
    for (int64_t b = 0; b < B; ++b) {
      active |= h_flags[(size_t)(2 * b)] < 0;
      any_bad |= h_flags[(size_t)(2 * B + b)] >= 0;
    }
  }
  DROP_HIP(hipMemcpyAsync(R, half[cur], (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(V, d_V, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(F_end, d_F, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(E_end, d_E, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(dt, d_dt, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(alpha, d_alpha, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(n_pos, d_npos, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(n_taken, d_ntaken, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipStreamSynchronize(st));
  memcpy(status, h_flags, (size_t)(2 * B) * 8);
  if (first_bad_step) memcpy(first_bad_step, h_flags + 2 * B, (size_t)B * 8);

  // evaluations made; a frozen replica repeats its last history values and its end positions up to there (the launches
  // behind its freeze wrote nothing for it)
  int64_t n_made = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t e = h_flags[(size_t)(2 * b + 1)];
    n_made = std::max(n_made, e < 0 ? t : e + 1);
  }
  for (int64_t b = 0; b < B; ++b) {
    const int64_t e = h_flags[(size_t)(2 * b + 1)];
    if (e < 0) continue;
    for (int64_t u = e + 1; u < n_made; ++u) {
      E_hist[u * B + b] = E_hist[e * B + b];
      fmax_hist[u * B + b] = fmax_hist[e * B + b];
      if (R_rec && u % record_every == 0) memcpy(R_rec + (u / record_every) * nc + b * n3, R + b * n3, (size_t)n3 * 8);
    }
  }
  return drop(GDML_OK);
}

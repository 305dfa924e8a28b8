// On-device molecular dynamics (gdml_md_run, gdml_md_noise; include/gdml_hip.h has the equations): positions, velocities
// and forces of B independent replicas stay in device memory for the whole run, the host sees recorded frames only.
//
// Two routes, the same arithmetic of a step on both, plain launches queued on the context's stream, stream order being the only
// dependency between steps:
//   single launch (D <= 256, at most 8 replicas): md_step_kernel, one kernel per step (see there)
//   general (every other shape; ring polymers, gdml_pimd_run in pimd.hip, have their own two kernels on this shape), three
//   pieces per step:
//     md_pre_kernel   half kick, drift (Langevin: half drift, Ornstein-Uhlenbeck step with Philox noise, half drift)
//     gdml_predict_dev on the new positions -- the library's device prediction path as it is (its route selection, its kernels)
//     md_post_kernel  second half kick, kinetic energy of each replica by a fixed tree, frame write on a recording step
// The host synchronises once per chunk of frames (bounded in bytes and in queued steps), copies the chunk out and reads the
// per-replica "first non-finite step" flags.  fp64 throughout, no atomics on floating-point values: results do not depend on
// chunking, on record_every or on how a run is cut into continued runs.
// The chunked driver, the noise and the reduction tree are traj.h's, shared with pimd.hip and relax.hip.
#include <math.h>

#include "common.h"
#include "fused_core.h"
#include "traj.h"

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
  __shared__ double red[1][256];
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
  red[0][t] = ek;
  if (nf) nonfinite = 1;
  __syncthreads();
  block_tree_sum<1>(red, t);
  if (t == 0) {
    const double e = E[b];
    Ekin[b] = red[0][0];
    if ((nonfinite || !isfinite(e)) && bad[b] < 0) bad[b] = step;
    if (fr.on) {
      fr.E[b] = e;
      fr.Ekin[b] = red[0][0];
    }
  }
}

// ------------------------------------------------------------------------------------------
// Single-launch step for the shapes of the single-launch predictor (D <= 256, B <= 8 replicas): ONE kernel per step on the
// core of predict_fused_kernel (fused_core.h) -- one row loop, row split, partial sum and back-projection -- except that
//   - the state (R, V, F) of step t comes from device memory (one half of a ping-pong buffer), not from the kernel arguments;
//   - every workgroup of a replica redoes the cheap first half of the step (md_first_half) to hold r_{t+1} in LDS.
// grid = (row shares, replicas).  The LAST workgroup of a replica to finish (ticket) sums that replica's partials in a fixed
// order, forms F_{t+1} = J^T F_x, finishes the velocity, sums the kinetic energy by the tree of md_post_kernel and writes
// R, V, F, E', E_kin of step t + 1 to the other half of the state buffer (and to the frame slot on a recording step).  No
// workgroup reads what another workgroup of the same launch writes; stream order is the only dependency between steps.
// init: no kick and no drift -- the forces of the start geometry by the same arithmetic, so that a continued run starts from
// the bits the run it continues ended with.
// ------------------------------------------------------------------------------------------
struct MdStepArgs {
  FusedModel M;
  int init;
  MdConst C;
  const double* mass;
  const double *inR, *inV, *inF;
  double *outR, *outV, *outF, *outE, *outEk;
  int64_t* bad;
  int64_t step;
  MdFrame fr;
};

template <int KPL>
__global__ void __launch_bounds__(256) md_step_kernel(MdStepArgs A) {
  __shared__ double s_fx[4][KPL * 64];  // per-wavefront F_x; reused by the replica's last workgroup: [0] = its summed F_x
  __shared__ double s_E[4];
  __shared__ double s_g[KPL * 64 * 3];
  __shared__ double s_r[FUSED_MAX_N3], s_v[FUSED_MAX_N3];
  __shared__ double s_red[1][256];
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

  if (!fused_partials<KPL>(A.M, (const double*)s_r, s_fx, s_E, s_ticket)) return;
  double* fxs = &s_fx[0][0];
  fused_sum_partials(A.M, fxs, [&](double e) { s_Eq = e; });
  fused_jacobian(A.M, (const double*)s_r, s_g);
  __syncthreads();
  double ek = 0.0;
  if (tid < n3) {  // F = J_x^T F_x, then the second half kick
    const int t = tid, a = t / 3;
    const double f = fused_force(N, s_g, fxs, t);
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
  s_red[0][tid] = ek;  // the tree of md_post_kernel: the same kinetic energy bit for bit
  __syncthreads();
  block_tree_sum<1>(s_red, tid);
  if (tid == 0) {
    const double e = s_Eq;
    A.outE[q] = e;
    A.outEk[q] = s_red[0][0];
    if ((s_nonfinite || !isfinite(e)) && A.bad[q] < 0) A.bad[q] = A.step;
    if (A.fr.on) {
      A.fr.E[q] = e;
      A.fr.Ekin[q] = s_red[0][0];
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

// argument checks shared by every route; ctx may be NULL (the message then goes where gdml_ctx_create's goes)
static int md_check(gdml_ctx* ctx, const gdml_md_params* p, const double* R, const double* V, int64_t n_steps,
                    int64_t record_every) {
  const char* fn = "gdml_md_run";
  GDML_TRY(traj_check_md_head(ctx, fn, p, n_steps, record_every));
  GDML_TRY(traj_check_shape(ctx, fn, p->B, p->N));
  GDML_TRY(traj_check_md_integrator(ctx, fn, p->N, p->dt, p->f_scale, p->mass, p->lat, p->lat_inv, p->thermostat, "Langevin"));
  if (!(p->gamma >= 0.0) || !isfinite(p->gamma)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: gamma < 0");
  if (!(p->kT >= 0.0) || !isfinite(p->kT)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_md_run: kT < 0");
  return traj_check_md_tail(ctx, fn, p->step0, R, V);
}

extern "C" int gdml_md_run(gdml_ctx* ctx, const gdml_md_params* p, double* R, double* V, int64_t n_steps, int64_t record_every,
                           double* R_rec, double* V_rec, double* F_rec, double* E_rec, double* Ekin_rec,
                           int64_t* first_bad_step) {
  GDML_TRY(md_check(ctx, p, R, V, n_steps, record_every));
  bool run;
  GDML_TRY(traj_prelude(ctx, "gdml_md_run", p->N, p->B, first_bad_step, &run));
  if (!run) return GDML_OK;
  Model& md = ctx->model;
  const int64_t B = p->B;
  const int n3 = 3 * p->N;
  const int64_t nc = B * n3;

  // E and E_kin of a recorded frame are written whether the caller wants them or not
  Recorder rec;
  const int f_R = rec.add(R_rec, nc), f_V = rec.add(V_rec, nc), f_F = rec.add(F_rec, nc);
  const int f_E = rec.add(E_rec, B, true), f_Ek = rec.add(Ekin_rec, B, true);
  rec.size(ctx, n_steps / record_every);  // 0: nothing is recorded (n_steps < record_every)

  // the single-launch step serves the shapes of the single-launch predictor
  const bool fused =
      fused_serves(md, B) && n3 <= FUSED_MAX_N3 && !ctx->profiling && ctx_opt_i(ctx, "predict.md_fused", 1) != 0;
  const FusedPlan plan = fused_plan(ctx, md);

  // one allocation: mass | two halves of the state (R | V | F | E | Ekin each; the general route works in the first) | bad |
  // frames of a chunk (R, V, F as requested, E, Ekin) | workgroup partials and tickets of the single-launch step
  const int64_t n_half = 3 * nc + 2 * B;
  const int64_t n_state = p->N + 2 * n_half + B;
  const int64_t n_part = fused ? fused_part_len(md, plan, B) + FUSED_MAX_Q : 0;
  double* buf = nullptr;
  GDML_TRY(ctx_alloc(ctx, (void**)&buf, (n_state + rec.len() + n_part) * 8));
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
  double* d_part = rec.carve(half[1] + n_half + B);
  unsigned* d_counter = (unsigned*)(d_part + fused_part_len(md, plan, B));

  hipStream_t st = ctx->stream;
  DROP_HIP(hipMemcpyAsync(d_mass, p->mass, (size_t)p->N * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_R, R, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_V, V, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  traj_fill_i64_kernel<<<ceil_div(B, 256), 256, 0, st>>>(d_bad, B, -1);
  if (fused) DROP_HIP(hipMemsetAsync(d_counter, 0, FUSED_MAX_Q * 8, st));
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
    fused_fill(S.M, md, plan, p->lat, p->lat_inv, d_part, d_counter);
    S.C = C; S.mass = d_mass; S.bad = d_bad;
  }
  // one single-launch step from the current half of the state into the other one
  auto launch_step = [&](int init, int64_t step, const MdFrame& fr) {
    const double* in = half[cur];
    double* out = half[cur ^ 1];
    S.init = init; S.step = step; S.fr = fr;
    S.inR = in; S.inV = in + nc; S.inF = in + 2 * nc;
    S.outR = out; S.outV = out + nc; S.outF = out + 2 * nc; S.outE = out + 3 * nc; S.outEk = out + 3 * nc + B;
    fused_launch(plan, B, st, md_step_kernel<1>, md_step_kernel<2>, md_step_kernel<4>, S);
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
  DROP_TRY(traj_run_chunks(ctx, rec, n_steps, record_every, d_bad, h_bad, [&](int64_t t, int64_t frame) {
    const int64_t step = p->step0 + t;
    MdFrame fr = {};
    if (frame >= 0)
      fr = MdFrame{rec.slot(f_R, frame), rec.slot(f_V, frame), rec.slot(f_F, frame), rec.slot(f_E, frame), rec.slot(f_Ek, frame), 1};
    if (fused) {
      launch_step(0, step, fr);
      return (int)GDML_OK;
    }
    md_pre_kernel<<<pre_grid, 256, 0, st>>>(C, d_mass, d_R, d_V, d_F, d_bad, step);
    // the timer of the previous step's prediction is dropped unread: reading it would wait for that step on the host
    ctx->phase_pending.clear();
    GDML_TRY(gdml_predict_dev(ctx, d_R, B, p->lat, p->lat_inv, d_E, d_F));
    md_post_kernel<<<(unsigned)B, 256, 0, st>>>(C, d_mass, d_R, d_V, d_F, d_E, d_Ek, d_bad, step, fr);
    return (int)GDML_OK;
  }));
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

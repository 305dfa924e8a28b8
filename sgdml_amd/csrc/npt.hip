// ------------------------------------------------------------------------------------------
// Constant-pressure molecular dynamics (gdml_npt_run): B independent replicas of a periodic model under the isotropic
// Martyna-Tobias-Klein equations, NPH or with a Langevin thermostat on the particles and on the piston.  Positions, velocities,
// forces, virial, log-scale eps and piston momentum stay in device memory; the host sees recorded frames only.  The contract
// (include/gdml_hip.h and tests/_npt_ref.py state the same).  Per replica: masses m, N_f = 3N, kappa = 1 + 3/N_f;
// f = f_scale F', Wv = f_scale W'; K = sum m v^2 / 2; reference lattice L0, V0 = |det L0|; state (r, v, eps, p_eps);
// lambda = exp(eps), L = lambda L0, L^-1 = L0^-1 / lambda, Vol = lambda^3 V0; alpha = p_eps / Wp (Wp = inf: exactly 0);
// G_eps = kappa 2K - tr Wv - 3 P_ext Vol.  Step t (step = step0 + t):
//   1. p_eps += dt/2 G_eps                                             (K, tr Wv, Vol of the current state)
//   2. s = exp(-kappa alpha dt/4):  v = s v;  v += dt/2 f/m;  v = s v
//   3. no thermostat:  q = exp(alpha dt/2):  r = q r;  r += dt v;  r = q r;  eps += alpha dt
//      Langevin:       q = exp(alpha dt/4):  r = q r;  r += dt/2 v;  r = q r;  eps += alpha dt/2
//                      v = c1 v + c2 sqrt(kT/m) xi_k;  p_eps = b1 p_eps + b2 sqrt(Wp kT) xi_3N;  alpha = p_eps / Wp
//                      the same half drift with the new alpha
//   4. E', F', W' = gdml_predict_virial_cells_dev(r, L, L^-1) for all B replicas
//   5. s = exp(-kappa alpha dt/4) with the current alpha:  v = s v;  v += dt/2 f/m;  v = s v
//   6. K by md_post_kernel's tree;  p_eps += dt/2 G_eps
// Three pieces per step: npt_pre_kernel (1-3; writes L and L^-1 for the predictor), the prediction as
// gdml_predict_virial_cells_dev runs it, npt_post_kernel (5-6, non-finite check, frame).  One workgroup of 256 per replica in
// both kernels; every thread computes the replica's scalars (alpha, s, q, the piston's noise) itself, thread 0 writes them.
// Forces, virial and K of the start come from the same predictor call and the same tree (npt_post_kernel with init = 1).
// There is no single-launch route: FusedModel (fused_core.h) holds one Lattice by value.
// Rounding: contraction is OFF in this file and every fused multiply-add is written out.  The kicks, the drifts, the
// Ornstein-Uhlenbeck step and the kinetic energy are the operations md.hip's kernels compile to, so that with alpha = 0
// (s = q = 1 exactly) a run is gdml_md_run's general route bit for bit.
// Prelude, recorder, chunk loop, noise and tree are traj.h's.
// ------------------------------------------------------------------------------------------
#include <math.h>

#include "common.h"
#include "traj.h"

#pragma clang fp contract(off)

struct NptConst {
  int n3;
  double dt, hdt;  // hdt = 0.5 * dt as md.hip forms it
  double f_scale, kappa, pressure, Wp;
  double c1, c2, kT, b1, b2w;  // b2w = b2 sqrt(Wp kT); 0 with piston_noise = 0
  int thermostat, piston_noise;
  uint64_t seed;
};

struct NptArrays {  // device memory
  const double* mass;         // (N)
  double *R, *V;              // (B,3N)
  double *eps, *p_eps;        // (B)
  const double *L0, *L0i, *V0;  // (B,9), (B,9), (B)
  double *L, *Li;             // (B,9): lattice and inverse of the current state, what the predictor reads
  const double *F, *E, *W;    // F' (B,3N), E' (B), W' (B,9) of the current state
  double* Ekin;               // (B)
  int64_t* bad;               // (B)
};

struct NptFrame {
  double *R, *V, *F, *lat;  // slot of the frame in the chunk buffers (null: not recorded)
  double* scal;             // (5,B): E', E_kin, Vol, P_int, p_eps
  int on;
};

__device__ __forceinline__ double npt_volume(double lam, double V0) { return lam * lam * lam * V0; }

__device__ __forceinline__ double npt_g_eps(const NptConst& C, double K, const double* w, double vol) {
  return C.kappa * (2.0 * K) - C.f_scale * (w[0] + w[4] + w[8]) - 3.0 * C.pressure * vol;
}

// steps 2 and 5 for one coordinate
__device__ __forceinline__ double npt_kick(const NptConst& C, double s, double m, double f, double v) {
  v = s * v;
  v = fma(C.hdt, C.f_scale * f / m, v);
  return s * v;
}

// the exact flow of r' = alpha r + v over h at fixed v and alpha, q = exp(alpha h / 2)
__device__ __forceinline__ double npt_drift(double q, double h, double v, double r) {
  r = q * r;
  r = fma(h, v, r);
  return q * r;
}

// L = lambda L0 and L^-1 = L0^-1 / lambda, entry by entry (threads 0 .. 8)
__device__ __forceinline__ void npt_write_cell(const NptArrays& A, int64_t b, double lam, int tid) {
  if (tid < 9) {
    A.L[b * 9 + tid] = lam * A.L0[b * 9 + tid];
    A.Li[b * 9 + tid] = A.L0i[b * 9 + tid] / lam;
  }
}

// before the first prediction: L and L^-1 of the start
__global__ void __launch_bounds__(256) npt_cell_kernel(NptArrays A) {
  const int64_t b = blockIdx.x;
  npt_write_cell(A, b, exp(A.eps[b]), threadIdx.x);
}

// one workgroup per replica: steps 1-3 of step `step` (absolute index)
__global__ void __launch_bounds__(256) npt_pre_kernel(NptConst C, NptArrays A, int64_t step) {
  const int64_t b = blockIdx.x;
  const int64_t o = b * C.n3;
  const int tid = threadIdx.x;
  double eps = A.eps[b], p = A.p_eps[b];
  const double K = A.Ekin[b];
  const double G = npt_g_eps(C, K, A.W + b * 9, npt_volume(exp(eps), A.V0[b]));
  __syncthreads();  // every thread has read the scalars thread 0 writes below
  p = p + C.hdt * G;
  double alpha = p / C.Wp;
  const double s = exp(-C.kappa * alpha * C.dt / 4.0);
  const double h = C.thermostat ? C.hdt : C.dt;
  const double q1 = exp(alpha * h / 2.0);
  eps = eps + alpha * h;
  double q2 = 1.0;
  if (C.thermostat) {
    if (C.piston_noise) p = C.b1 * p + C.b2w * md_normal(C.seed, (uint64_t)step, (uint32_t)b, C.n3);
    alpha = p / C.Wp;
    q2 = exp(alpha * h / 2.0);
    eps = eps + alpha * h;
  }
  int nf = 0;
  for (int k = tid; k < C.n3; k += 256) {
    const double m = A.mass[k / 3];
    double v = npt_kick(C, s, m, A.F[o + k], A.V[o + k]);
    double r = npt_drift(q1, h, v, A.R[o + k]);
    if (C.thermostat) {
      const double xi = md_normal(C.seed, (uint64_t)step, (uint32_t)b, k);
      v = fma(C.c1, v, C.c2 * sqrt(C.kT / m) * xi);
      r = npt_drift(q2, h, v, r);
    }
    A.R[o + k] = r;
    A.V[o + k] = v;
    nf |= !(isfinite(r) && isfinite(v));
  }
  const double lam = exp(eps);
  npt_write_cell(A, b, lam, tid);
  if (tid == 0) {
    A.eps[b] = eps;
    A.p_eps[b] = p;
    nf |= !(isfinite(eps) && isfinite(p) && isfinite(npt_volume(lam, A.V0[b])));
  }
  // every thread of a replica that finds the flag unset writes the same value: no ordering needed
  if (nf && A.bad[b] < 0) A.bad[b] = step;
}

// one workgroup per replica: steps 5-6 (init: neither, only K of the start), kinetic energy (per-thread partial sums in index
// order, then the fixed tree), non-finite check of the new forces and virial, frame write
__global__ void __launch_bounds__(256) npt_post_kernel(NptConst C, NptArrays A, int init, int64_t step, NptFrame fr) {
  __shared__ double red[1][256];
  __shared__ int nonfinite;
  const int64_t b = blockIdx.x;
  const int64_t o = b * C.n3;
  const int t = threadIdx.x;
  if (t == 0) nonfinite = 0;
  const double eps = A.eps[b];
  double p = A.p_eps[b];
  const double s = exp(-C.kappa * (p / C.Wp) * C.dt / 4.0);
  __syncthreads();
  double ek = 0.0;
  int nf = 0;
  for (int k = t; k < C.n3; k += 256) {
    const double m = A.mass[k / 3];
    const double f = A.F[o + k];
    double v = A.V[o + k];
    if (!init) {
      v = npt_kick(C, s, m, f, v);
      A.V[o + k] = v;
    }
    ek = fma(0.5 * m * v, v, ek);
    nf |= !(isfinite(v) && isfinite(f));
    if (fr.on) {
      if (fr.R) fr.R[o + k] = A.R[o + k];
      if (fr.V) fr.V[o + k] = v;
      if (fr.F) fr.F[o + k] = f;
    }
  }
  if (fr.on && fr.lat && t < 9) fr.lat[b * 9 + t] = A.L[b * 9 + t];
  red[0][t] = ek;
  if (nf) nonfinite = 1;
  __syncthreads();
  block_tree_sum<1>(red, t);
  if (t == 0) {
    const double K = red[0][0];
    const double e = A.E[b];
    const double* w = A.W + b * 9;
    const double vol = npt_volume(exp(eps), A.V0[b]);
    const double G = npt_g_eps(C, K, w, vol);
    if (!init) {
      p = p + C.hdt * G;
      A.p_eps[b] = p;
    }
    A.Ekin[b] = K;
    if ((nonfinite || !isfinite(e) || !isfinite(G) || !isfinite(p) || !isfinite(eps) || !isfinite(vol)) && A.bad[b] < 0)
      A.bad[b] = step;
    if (fr.on) {
      const int64_t B = gridDim.x;
      fr.scal[b] = e;
      fr.scal[B + b] = K;
      fr.scal[2 * B + b] = vol;
      fr.scal[3 * B + b] = (2.0 * K - C.f_scale * (w[0] + w[4] + w[8])) / (3.0 * vol);
      fr.scal[4 * B + b] = p;
    }
  }
}

// determinant in the order of gdml_cell_relax_run's header text
static double npt_det3(const double* a) {
  return a[0] * (a[4] * a[8] - a[5] * a[7]) + a[1] * (a[5] * a[6] - a[3] * a[8]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
}

// argument checks; ctx may be NULL (the message then goes where gdml_ctx_create's goes)
static int npt_check(gdml_ctx* ctx, const gdml_npt_params* p, const double* R, const double* V, const double* eps,
                     const double* p_eps, const double* L0, const double* L0_inv, int64_t n_steps, int64_t record_every) {
  const char* fn = "gdml_npt_run";
  GDML_TRY(traj_check_md_head(ctx, fn, p, n_steps, record_every));
  GDML_TRY(traj_check_shape(ctx, fn, p->B, p->N));
  GDML_TRY(traj_check_md_integrator(ctx, fn, p->N, p->dt, p->f_scale, p->mass, nullptr, nullptr, p->thermostat, "Langevin"));
  if (!(p->gamma >= 0.0) || !isfinite(p->gamma)) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: gamma < 0", fn);
  if (!(p->kT >= 0.0) || !isfinite(p->kT)) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: kT < 0", fn);
  if (!(p->gamma_baro >= 0.0) || !isfinite(p->gamma_baro)) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: gamma_baro < 0", fn);
  if (!(p->piston_mass > 0.0)) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: piston_mass must be positive (inf allowed)", fn);
  if (!isfinite(p->pressure)) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: pressure is not finite", fn);
  GDML_TRY(traj_check_md_tail(ctx, fn, p->step0, R, V));
  if (!eps || !p_eps) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: eps or p_eps is NULL", fn);
  if (!L0 || !L0_inv) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: L0 or L0_inv is NULL (NPT needs a lattice per replica)", fn);
  return GDML_OK;
}

extern "C" int gdml_npt_run(gdml_ctx* ctx, const gdml_npt_params* p, double* R, double* V, double* eps, double* p_eps,
                            const double* L0, const double* L0_inv, int64_t n_steps, int64_t record_every, double* R_rec,
                            double* V_rec, double* F_rec, double* lat_rec, double* E_rec, double* Ekin_rec, double* vol_rec,
                            double* press_rec, double* peps_rec, int64_t* first_bad_step) {
  GDML_TRY(npt_check(ctx, p, R, V, eps, p_eps, L0, L0_inv, n_steps, record_every));
  bool run;
  GDML_TRY(traj_prelude(ctx, "gdml_npt_run", p->N, p->B, first_bad_step, &run));
  if (!run || n_steps == 0) return GDML_OK;
  const int64_t B = p->B;
  const int n3 = 3 * p->N;
  const int64_t nc = B * n3;

  // the five per-replica scalars of a frame travel as ONE field (5,B) and are dealt to the caller's arrays behind the run
  const int64_t n_rec = n_steps / record_every;
  double* const scal_out[5] = {E_rec, Ekin_rec, vol_rec, press_rec, peps_rec};
  bool want_scal = false;
  for (double* a : scal_out) want_scal |= a != nullptr;
  std::vector<double> h_scal(want_scal ? (size_t)(n_rec * 5 * B) : 0);
  Recorder rec;
  const int f_R = rec.add(R_rec, nc), f_V = rec.add(V_rec, nc), f_F = rec.add(F_rec, nc), f_L = rec.add(lat_rec, 9 * B);
  const int f_S = rec.add(want_scal && n_rec > 0 ? h_scal.data() : nullptr, 5 * B, true);
  rec.size(ctx, n_rec);  // 0: nothing is recorded (n_steps < record_every)

  // one allocation: mass | R | V | F' | L | L^-1 | L0 | L0^-1 | W' | eps | p_eps | V0 | E' | Ekin | bad | frames of a chunk
  const int64_t n_state = p->N + 3 * nc + 5 * 9 * B + 6 * B;
  double* buf = nullptr;
  GDML_TRY(ctx_alloc(ctx, (void**)&buf, (n_state + rec.len()) * 8));
  auto drop = [&](int rc) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)ctx_free(ctx, buf);
    return rc;
  };
  double* d_mass = buf;
  double* d_R = d_mass + p->N;
  double* d_V = d_R + nc;
  double* d_F = d_V + nc;
  double* d_L = d_F + nc;
  double* d_Li = d_L + 9 * B;
  double* d_L0 = d_Li + 9 * B;
  double* d_L0i = d_L0 + 9 * B;
  double* d_W = d_L0i + 9 * B;
  double* d_eps = d_W + 9 * B;
  double* d_peps = d_eps + B;
  double* d_V0 = d_peps + B;
  double* d_E = d_V0 + B;
  double* d_Ek = d_E + B;
  int64_t* d_bad = (int64_t*)(d_Ek + B);
  rec.carve(d_Ek + 2 * B);

  std::vector<double> h_V0((size_t)B);
  for (int64_t b = 0; b < B; ++b) h_V0[(size_t)b] = fabs(npt_det3(L0 + 9 * b));

  hipStream_t st = ctx->stream;
  DROP_HIP(hipMemcpyAsync(d_mass, p->mass, (size_t)p->N * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_R, R, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_V, V, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_L0, L0, (size_t)B * 72, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_L0i, L0_inv, (size_t)B * 72, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_eps, eps, (size_t)B * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_peps, p_eps, (size_t)B * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_V0, h_V0.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
  traj_fill_i64_kernel<<<ceil_div(B, 256), 256, 0, st>>>(d_bad, B, -1);
  // the caller's arrays are pageable: the copies above have to be through before they may change
  DROP_HIP(hipStreamSynchronize(st));

  NptConst C;
  C.n3 = n3;
  C.dt = p->dt;
  C.hdt = 0.5 * p->dt;
  C.f_scale = p->f_scale;
  C.kappa = 1.0 + 3.0 / (double)n3;
  C.pressure = p->pressure;
  C.Wp = p->piston_mass;
  C.thermostat = p->thermostat;
  C.c1 = exp(-p->gamma * p->dt);
  C.c2 = sqrt(1.0 - C.c1 * C.c1);
  C.kT = p->kT;
  C.b1 = exp(-p->gamma_baro * p->dt);
  C.piston_noise = p->thermostat && isfinite(p->piston_mass);
  C.b2w = C.piston_noise ? sqrt(1.0 - C.b1 * C.b1) * sqrt(p->piston_mass * p->kT) : 0.0;
  C.seed = p->seed;
  const NptArrays A = {d_mass, d_R, d_V, d_eps, d_peps, d_L0, d_L0i, d_V0, d_L, d_Li, d_F, d_E, d_W, d_Ek, d_bad};

  // forces, virial and kinetic energy of the start (a continued run recomputes them from its predecessor's end state by the
  // same arithmetic: the same bits)
  npt_cell_kernel<<<(unsigned)B, 256, 0, st>>>(A);
  ctx->phase_pending.clear();
  DROP_TRY(gdml_predict_virial_cells_dev(ctx, d_R, B, d_L, d_Li, d_E, d_F, d_W));
  npt_post_kernel<<<(unsigned)B, 256, 0, st>>>(C, A, 1, p->step0, NptFrame{});

  std::vector<int64_t> h_bad((size_t)B);
  DROP_TRY(traj_run_chunks(ctx, rec, n_steps, record_every, d_bad, h_bad, [&](int64_t t, int64_t frame) {
    const int64_t step = p->step0 + t;
    NptFrame fr = {};
    if (frame >= 0)
      fr = NptFrame{rec.slot(f_R, frame), rec.slot(f_V, frame), rec.slot(f_F, frame), rec.slot(f_L, frame), rec.slot(f_S, frame), 1};
    npt_pre_kernel<<<(unsigned)B, 256, 0, st>>>(C, A, step);
    // the timer of the previous step's prediction is dropped unread: reading it would wait for that step on the host
    ctx->phase_pending.clear();
    GDML_TRY(gdml_predict_virial_cells_dev(ctx, d_R, B, d_L, d_Li, d_E, d_F, d_W));
    npt_post_kernel<<<(unsigned)B, 256, 0, st>>>(C, A, 0, step, fr);
    return (int)GDML_OK;
  }));
  DROP_HIP(hipMemcpyAsync(R, d_R, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(V, d_V, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(eps, d_eps, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(p_eps, d_peps, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipStreamSynchronize(st));
  if (first_bad_step) memcpy(first_bad_step, h_bad.data(), (size_t)B * 8);
  for (int64_t k = 0; k < rec.done; ++k)
    for (int c = 0; c < 5; ++c)
      if (scal_out[c]) memcpy(scal_out[c] + k * B, h_scal.data() + (k * 5 + c) * B, (size_t)B * 8);
  return drop(GDML_OK);
}

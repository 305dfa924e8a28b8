// ------------------------------------------------------------------------------------------
// Path-integral MD (gdml_pimd_run, gdml_pimd_modes; include/gdml_hip.h has the equations): B rings of P beads, state
// (B, P, 3N).  The general route's shape -- three pieces per step, stream order the only dependency:
//   pimd_pre_kernel   half kick of every bead, orthonormal real DFT over the bead index, exact free ring-polymer flow (PILE-L:
//                     half flow, Ornstein-Uhlenbeck step in mode space, half flow), transform back
//   gdml_predict_dev  on all B P geometries as one batch
//   pimd_post_kernel  second half kick, centroid, the five ring quantities by fixed trees, frame write on a recording step
// Rings always take this route (a single-launch ring step does not exist).  The chunked driver, the noise and the reduction
// tree are traj.h's, shared with md.hip and relax.hip.
// ------------------------------------------------------------------------------------------
#include <math.h>

#include "common.h"
#include "traj.h"

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
// E_kin, E_spring and sum_j (r_j - r_c) F'_j in that fixed order, then the 256-slot tree (block_tree_sum) for each
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
  block_tree_sum<3>(red, t);
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
  const char* fn = "gdml_pimd_run";
  GDML_TRY(traj_check_md_head(ctx, fn, p, n_steps, record_every));
  GDML_TRY(traj_check_shape(ctx, fn, p->B, p->N));
  if (p->beads < 1 || p->beads > PIMD_MAX_BEADS) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: beads outside 1..128");
  if (p->B * p->beads > 0x7fffffffLL) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: B * beads must stay below 2^31");
  GDML_TRY(traj_check_md_integrator(ctx, fn, p->N, p->dt, p->f_scale, p->mass, p->lat, p->lat_inv, p->thermostat, "PILE-L"));
  if (!(p->gamma_centroid >= 0.0) || !isfinite(p->gamma_centroid))
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: gamma_centroid < 0");
  if (!(p->pile_lambda > 0.0) || !isfinite(p->pile_lambda))
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: pile_lambda must be positive and finite");
  if (!(p->kT >= 0.0) || !isfinite(p->kT)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: kT < 0");
  if (p->beads > 1 && !(p->kT > 0.0)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: kT must be positive with more than one bead");
  if (!(p->hbar > 0.0) || !isfinite(p->hbar)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_pimd_run: hbar must be positive and finite");
  return traj_check_md_tail(ctx, fn, p->step0, R, V);
}

extern "C" int gdml_pimd_run(gdml_ctx* ctx, const gdml_pimd_params* p, double* R, double* V, int64_t n_steps, int64_t record_every,
                             double* R_rec, double* V_rec, double* F_rec, double* E_rec, double* Rc_rec, double* ring_rec,
                             int64_t* first_bad_step) {
  GDML_TRY(pimd_check(ctx, p, R, V, n_steps, record_every));
  bool run;
  GDML_TRY(traj_prelude(ctx, "gdml_pimd_run", p->N, p->B, first_bad_step, &run));
  if (!run) return GDML_OK;
  const int64_t B = p->B;
  const int P = p->beads, n3 = 3 * p->N;

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
  // the ring quantities of a recorded frame are written whether the caller wants them or not
  Recorder rec;
  const int f_R = rec.add(R_rec, nc), f_V = rec.add(V_rec, nc), f_F = rec.add(F_rec, nc), f_E = rec.add(E_rec, BP);
  const int f_Rc = rec.add(Rc_rec, B * n3), f_ring = rec.add(ring_rec, 5 * B, true);
  rec.size(ctx, n_steps / record_every);  // 0: nothing is recorded (n_steps < record_every)

  // one allocation: mass | C | C^T | mode table | R | V | F | E | bad | frames of a chunk (R, V, F, E, Rc as requested, ring)
  const int64_t n_tab = p->N + 2 * (int64_t)P * P + 5 * P;
  const int64_t n_state = n_tab + 3 * nc + BP + B;
  double* buf = nullptr;
  GDML_TRY(ctx_alloc(ctx, (void**)&buf, (n_state + rec.len()) * 8));
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
  rec.carve(d_E + BP + B);

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
  traj_fill_i64_kernel<<<ceil_div(B, 256), 256, 0, st>>>(d_bad, B, -1);
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
  DROP_TRY(traj_run_chunks(ctx, rec, n_steps, record_every, d_bad, h_bad, [&](int64_t t, int64_t frame) {
    const int64_t step = p->step0 + t;
    pre<<<pre_grid, T, pre_lds, st>>>(C, d_mass, d_Cm, d_Ct, d_coef, d_R, d_V, d_F, d_bad, step);
    // the timer of the previous step's prediction is dropped unread: reading it would wait for that step on the host
    ctx->phase_pending.clear();
    GDML_TRY(gdml_predict_dev(ctx, d_R, BP, p->lat, p->lat_inv, d_E, d_F));
    PimdFrame fr = {};
    if (frame >= 0)
      fr = PimdFrame{rec.slot(f_R, frame), rec.slot(f_V, frame), rec.slot(f_F, frame), rec.slot(f_E, frame),
                     rec.slot(f_Rc, frame), rec.slot(f_ring, frame), 1};
    pimd_post_kernel<<<(unsigned)B, 256, 0, st>>>(C, d_mass, d_R, d_V, d_F, d_E, d_bad, step, fr);
    return (int)GDML_OK;
  }));
  DROP_HIP(hipMemcpyAsync(R, d_R, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(V, d_V, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipStreamSynchronize(st));
  if (first_bad_step && n_steps > 0) memcpy(first_bad_step, h_bad.data(), (size_t)B * 8);
  return drop(GDML_OK);
}

// ------------------------------------------------------------------------------------------
// Nudged elastic band (gdml_neb_run): B independent bands of P images between two fixed end points relax to the minimum-energy
// path by FIRE, a whole band being ONE FIRE system (one v, dt, alpha, n_pos, n_taken per band), as ASE drives FIRE(NEB(...)).
// The step (the contract; include/gdml_hip.h and tests/_neb_ref.py state the same):
//   g = f_scale F'; E' the predictor's unscaled energy; images 0 and P - 1 never move.  Evaluation t = 0, 1, ... of an active band:
//   1. E', F' = predictor of all P images (the end points' are computed and not used for motion)
//   2. for every interior image i, tau+ = r_{i+1} - r_i, tau- = r_i - r_{i-1} (plain differences):
//        E_{i+1} > E_i > E_{i-1}: tau = tau+;   E_{i+1} < E_i < E_{i-1}: tau = tau-;   otherwise, with dE_max, dE_min the larger and
//        the smaller of |E_{i+1} - E_i|, |E_{i-1} - E_i|: tau = tau+ dE_max + tau- dE_min if E_{i+1} > E_{i-1}, else
//        tau = tau+ dE_min + tau- dE_max;   tau^ = tau / |tau|
//        F_i = g_i - (g_i . tau^) tau^ + k (|tau+| - |tau-|) tau^
//        climb: the interior image of highest E' (ties: the lowest index; chosen anew at every evaluation) gets
//        F_i = g_i - 2 (g_i . tau^) tau^ instead
//   3. f_atom = max over interior images and atoms |F_{i,atom}|;  f_atom < fmax: converged;  else t = max_steps: stops unconverged;
//      a frozen band is never written again
//   4. else gdml_relax_run's update 4 on the band vector of (P - 2) 3N coordinates with F in place of g
// Sums: per-thread partial sums in index order, then the 256-slot tree (block_tree_sum, traj.h); no floating-point atomics.
// Three pieces per evaluation, ordered by the stream alone:
//   gdml_predict_dev   all B P geometries as one batch
//   neb_force_kernel   one workgroup per interior image: tangent, the four per-image sums, F_i into the band force buffer; with
//                      climb it finds the highest image itself from the band's energies (a fixed tree, no broadcast)
//   neb_step_kernel    one workgroup per band: relax_finish (relax_finish.h) on the band vector, history, frame, status; on freeze
//                      the end-of-run outputs
// Checks, prelude, recorder and the chunk loop are traj.h's, shared with relax.hip.
// ------------------------------------------------------------------------------------------
#include <math.h>

#include "common.h"
#include "traj.h"
#include "relax_finish.h"

#define NEB_MAX_IMAGES 128

struct NebBand {  // what both kernels know of the bands
  int P, n3;
  const double* R;   // (B,P,3N)
  const double* Ft;  // (B,P,3N) F' of this evaluation
  const double* Et;  // (B,P) E'
  double* Fb;        // (B,P,3N) the NEB force; rows 0 and P - 1 of a band are never touched
  double* ftan;      // (B,P) scratch: g . tau^ of the interior images
  double* inc;       // (B,P) scratch: [i] = |r_i - r_{i-1}|, i = 1 .. P - 1
  const int64_t* status;
};

// The interior image of highest E' (ties: the lowest index) of a band with energies E (P of them), found by every workgroup
// that needs it on its own: the first 128 threads load one energy each (one round of loads instead of P dependent ones), then a
// tree over the 128 slots of s_e, s_i; a slot outside the interior holds (-inf, image 1).  Called by all 256 threads; every
// thread gets the result.
__device__ __forceinline__ int neb_highest(const double* E, int P, double* s_e, int* s_i, int tid) {
  if (tid < NEB_MAX_IMAGES) {
    const bool in = tid >= 1 && tid < P - 1;
    s_e[tid] = in ? E[tid] : -INFINITY;
    s_i[tid] = in ? tid : 1;
  }
  __syncthreads();
  for (int s = NEB_MAX_IMAGES / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const double el = s_e[tid], er = s_e[tid + s];
      const int il = s_i[tid], ir = s_i[tid + s];
      if (er > el || (er == el && ir < il)) {
        s_e[tid] = er;
        s_i[tid] = ir;
      }
    }
    __syncthreads();
  }
  return s_i[0];
}

// step 2 for one interior image: grid = B (P - 2), image i = 1 + blockIdx.x % (P - 2) of band blockIdx.x / (P - 2).  Reads r and
// E' of the image and its neighbours (written by earlier launches); writes nothing another workgroup of this launch reads.
__global__ void __launch_bounds__(256) neb_force_kernel(NebBand A, double f_scale, double k_spring, int climb) {
  __shared__ double red[4][256];
  __shared__ double s_e[NEB_MAX_IMAGES];
  __shared__ int s_i[NEB_MAX_IMAGES];
  const int tid = threadIdx.x, P = A.P, n3 = A.n3;
  const int64_t q = blockIdx.x / (unsigned)(P - 2);
  if (A.status[2 * q] >= 0) return;
  const int i = 1 + (int)(blockIdx.x % (unsigned)(P - 2));
  const int64_t img = q * P + i;
  const double* E = A.Et + q * P;
  const double *r0 = A.R + (img - 1) * n3, *r1 = r0 + n3, *r2 = r1 + n3;
  const double* f = A.Ft + img * n3;

  const double em = E[i - 1], e0 = E[i], ep = E[i + 1];
  double a, b;  // tau = a tau+ + b tau-
  if (ep > e0 && e0 > em) {
    a = 1.0;
    b = 0.0;
  } else if (ep < e0 && e0 < em) {
    a = 0.0;
    b = 1.0;
  } else {
    const double dp = fabs(ep - e0), dm = fabs(em - e0);
    const double d_max = dp > dm ? dp : dm, d_min = dp > dm ? dm : dp;
    a = ep > em ? d_max : d_min;
    b = ep > em ? d_min : d_max;
  }
  const bool climbs = climb && i == neb_highest(E, P, s_e, s_i, tid);  // (climb is the same in every thread)

  double gt = 0.0, pp = 0.0, mm = 0.0, tt = 0.0;
  for (int k = tid; k < n3; k += 256) {
    const double tp = r2[k] - r1[k], tm = r1[k] - r0[k];
    const double tau = a * tp + b * tm, g = f_scale * f[k];
    gt += g * tau;
    pp += tp * tp;
    mm += tm * tm;
    tt += tau * tau;
  }
  red[0][tid] = gt;
  red[1][tid] = pp;
  red[2][tid] = mm;
  red[3][tid] = tt;
  __syncthreads();
  block_tree_sum<4>(red, tid);
  const double len_p = sqrt(red[1][0]), len_m = sqrt(red[2][0]), len_t = sqrt(red[3][0]);
  const double dot = red[0][0] / len_t;  // g . tau^
  const double c = climbs ? -2.0 * dot / len_t : (k_spring * (len_p - len_m) - dot) / len_t;
  double* F = A.Fb + img * n3;
  for (int k = tid; k < n3; k += 256) {
    const double tp = r2[k] - r1[k], tm = r1[k] - r0[k];
    const double tau = a * tp + b * tm, g = f_scale * f[k];
    F[k] = g + c * tau;
  }
  if (tid == 0) {
    A.ftan[img] = dot;
    A.inc[img] = len_m;
    if (i == P - 2) A.inc[img + 1] = len_p;
  }
}

struct NebEnd {  // end-of-run outputs in device memory, written when a band freezes
  double *F, *E;  // (B,P,3N), (B,P): F', E' of the band's last evaluation
  double *s, *ftan;  // (B,P)
  int64_t* i_climb;  // (B)
};

// steps 3 and 4 for one band, one workgroup per band: relax_finish on the band vector (the interior images are contiguous in
// R, V and the band force buffer: element (q P + 1) 3N onwards), E'(highest interior image) and f_atom into the history
__global__ void __launch_bounds__(256) neb_step_kernel(RelaxConst C, RelaxState S, RelaxSlot sl, NebBand A, NebEnd Z, double* R,
                                                       int64_t t, int last) {
  __shared__ double red[4][256];
  __shared__ double s_e[NEB_MAX_IMAGES];
  __shared__ int s_i[NEB_MAX_IMAGES];
  const int64_t q = blockIdx.x;
  if (S.status[2 * q] >= 0) return;
  const int tid = threadIdx.x, P = A.P, n3 = A.n3;
  const int64_t img0 = q * P, o = (img0 + 1) * n3, o_last = (img0 + P - 1) * n3;
  const double* E = A.Et + img0;
  const int ic = neb_highest(E, P, s_e, s_i, tid);
  const int fin = __syncthreads_and(tid < P ? (int)isfinite(E[tid]) : 1);
  const double e = fin ? s_e[0] : NAN;  // a non-finite E' anywhere in the band marks it (relax_finish tests e)
  if (sl.R)  // the end points of the frame; relax_finish writes the interior
    for (int k = tid; k < n3; k += 256) {
      sl.R[img0 * n3 + k] = R[img0 * n3 + k];
      sl.R[o_last + k] = R[o_last + k];
    }
  double* r = R + o;
  if (!relax_finish(C, S, sl, q, t, last, r, A.Fb + o, e, r, nullptr, red, C.n3, o)) return;
  // frozen from here on: the band's outputs
  for (int64_t k = tid; k < (int64_t)P * n3; k += 256) Z.F[img0 * n3 + k] = A.Ft[img0 * n3 + k];
  for (int i = tid; i < P; i += 256) {
    Z.E[img0 + i] = E[i];
    Z.ftan[img0 + i] = (i == 0 || i == P - 1) ? 0.0 : A.ftan[img0 + i];
  }
  if (tid == 0) {
    double s = 0.0;
    Z.s[img0] = 0.0;
    for (int i = 1; i < P; ++i) {
      s += A.inc[img0 + i];
      Z.s[img0 + i] = s;
    }
    Z.i_climb[q] = ic;
  }
}

extern "C" int gdml_neb_run(gdml_ctx* ctx, const gdml_neb_params* p, double* R, double* V, double* dt, double* alpha,
                            int64_t* n_pos, int64_t* n_taken, int64_t max_steps, int64_t record_every, double* R_rec,
                            double* Emax_hist, double* fmax_hist, double* E_end, double* F_end, int64_t* i_climb, double* s,
                            double* f_tangent, int64_t* status, int64_t* first_bad_step) {
  const char* fn = "gdml_neb_run";
  if (!p) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: params is NULL", fn);
  if (p->P < 3 || p->P > NEB_MAX_IMAGES) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: P outside 3 ... %d", fn, NEB_MAX_IMAGES);
  if (!(p->k_spring > 0.0) || !isfinite(p->k_spring))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: k_spring must be positive and finite", fn);
  if (p->B > 0 && p->B * (int64_t)p->P > 0x7fffffffLL) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: B P out of range", fn);
  const FireParams fire = fire_params(*p);
  const FireState h_fire = {dt, alpha, n_pos, n_taken};
  GDML_TRY(relax_check(ctx, fn, p->B, p->N, p->f_scale, p->lat, p->lat_inv, fire, R, V, h_fire, max_steps, record_every, R_rec,
                       Emax_hist, fmax_hist, E_end, F_end, status));
  if (!i_climb || !s || !f_tangent)
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: an output array (i_climb, s, f_tangent) is NULL", fn);
  bool run;
  GDML_TRY(traj_prelude(ctx, fn, p->N, p->B, first_bad_step, &run));
  if (!run) return GDML_OK;
  const int64_t B = p->B;
  const int P = p->P, n3 = 3 * p->N;
  const int64_t nb = B * P, nc = nb * n3;
  FrozenRun fr = {B, max_steps, record_every, traj_frozen_chunk_steps(ctx, max_steps), 2, {Emax_hist, fmax_hist}};
  Recorder rec;
  const int f_R = rec.add(R_rec, nc);
  rec.size(ctx, fr.chunk_steps);

  // one allocation: R | V | band force | F', E' of the prediction | the outputs F, E, s, f_tangent, i_climb | scratch f_tangent,
  // arc-length increments | E'(highest image) | dt, alpha, n_pos, n_taken | status, bad, a chunk of the history | a chunk of frames
  const int64_t n_state = 5 * nc + 6 * nb + 6 * B;
  double* buf = nullptr;
  GDML_TRY(ctx_alloc(ctx, (void**)&buf, (n_state + fr.words() + rec.len()) * 8));
  auto drop = [&](int rc) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)ctx_free(ctx, buf);
    return rc;
  };
  double* d_R = buf;
  double* d_V = d_R + nc;
  double* d_Fb = d_V + nc;
  double* d_Ft = d_Fb + nc;
  double* d_F = d_Ft + nc;
  double* d_Et = d_F + nc;
  double* d_E = d_Et + nb;
  double* d_s = d_E + nb;
  double* d_ftan = d_s + nb;
  double* w_ftan = d_ftan + nb;
  double* w_inc = w_ftan + nb;
  int64_t* d_iclimb = (int64_t*)(w_inc + nb);
  double* d_Emax = (double*)(d_iclimb + B);
  FireState d_fire;
  rec.carve(fr.carve(d_fire.carve(d_Emax + B, B)));

  hipStream_t st = ctx->stream;
  DROP_HIP(hipMemcpyAsync(d_R, R, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_V, V, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(d_fire.copy(h_fire, B, false, st));
  // band force (its end rows are never written), outputs and scratch: zero
  DROP_HIP(hipMemsetAsync(d_Fb, 0, (size_t)(3 * nc + 6 * nb + B) * 8, st));
  // the caller's arrays are pageable: the copies above have to be through before they may change
  DROP_HIP(hipStreamSynchronize(st));

  // the band vector; the NEB force is built from g = f_scale F' already
  const RelaxConst C = relax_const(fire, (P - 2) * n3, 1.0);
  // relax_finish keeps "F'" of the vector in S.F: here the band force buffer itself (every thread rewrites what it read)
  RelaxState S = {d_V, d_Fb, d_Emax, d_fire.dt, d_fire.alpha, d_fire.n_pos, d_fire.n_taken, fr.status(), fr.bad()};
  NebBand A = {P, n3, d_R, d_Ft, d_Et, d_Fb, w_ftan, w_inc, fr.status()};
  NebEnd Z = {d_F, d_E, d_s, d_ftan, d_iclimb};

  DROP_TRY(traj_run_until_frozen(ctx, rec, R_rec != nullptr, fr, [&](int64_t te, int64_t row, int64_t frame, int last) {
    RelaxSlot sl = {fr.row(0, row), fr.row(1, row), frame >= 0 ? rec.slot(f_R, frame) : nullptr};
    // the timer of the previous evaluation's prediction is dropped unread: reading it would wait for it on the host
    ctx->phase_pending.clear();
    GDML_TRY(gdml_predict_dev(ctx, d_R, nb, p->lat, p->lat_inv, d_Et, d_Ft));
    neb_force_kernel<<<(unsigned)(B * (P - 2)), 256, 0, st>>>(A, p->f_scale, p->k_spring, p->climb != 0);
    neb_step_kernel<<<(unsigned)B, 256, 0, st>>>(C, S, sl, A, Z, d_R, te, last);
    return (int)GDML_OK;
  }));
  DROP_HIP(hipMemcpyAsync(R, d_R, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(V, d_V, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(F_end, d_F, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(E_end, d_E, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(s, d_s, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(f_tangent, d_ftan, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(i_climb, d_iclimb, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(d_fire.copy(h_fire, B, true, st));
  DROP_HIP(hipStreamSynchronize(st));
  const TrajFrames frames = {R_rec, R, (int64_t)P * n3};
  fr.finish(status, first_bad_step, &frames, 1);
  return drop(GDML_OK);
}

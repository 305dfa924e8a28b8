// The FIRE update of gdml_relax_run (relax.hip, which states the step) as one device function, shared with gdml_neb_run
// (neb.hip), where a whole band is one FIRE system.
#pragma once
#include <math.h>

#include "common.h"
#include "traj.h"

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

// Steps 1-4 for replica q once its F' is known, called by all 256 threads of one workgroup.  The replica's vector has n3
// coordinates (n3 / 3 atoms) and starts at element o of S.V, S.F and the frame sl.R: n3 = 3N, o = q 3N for a geometry; a band of
// gdml_neb_run (neb.hip) passes its (P - 2) 3N interior coordinates and the NEB force.  r: positions of this evaluation,
// fp: F', e: E'; r_next: where r(t+1) goes (may be r itself: every coordinate is read and written by one thread); r_keep: where
// a freezing replica's r is written as well (null: nowhere).  red: 4 x 256 doubles of LDS.  Returns whether the replica froze
// (the same value in every thread).
__device__ __forceinline__ bool relax_finish(const RelaxConst& C, const RelaxState& S, const RelaxSlot& sl, int64_t q, int64_t t,
                                             int last, const double* r, const double* fp, double e, double* r_next,
                                             double* r_keep, double (&red)[4][256], int n3, int64_t o) {
  const int tid = threadIdx.x;
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
  block_tree_sum<3, 1>(red, tid);
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
    return true;
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
  block_tree_sum<1>(red, tid);
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
  return false;
}

// ---- host side: what gdml_relax_run, gdml_neb_run and gdml_cell_relax_run share around the kernels -------------------------------
struct FireParams {  // the FIRE constants of gdml_relax_params, gdml_neb_params and gdml_cell_relax_params
  double fmax, dt_max, max_step, f_inc, f_dec, alpha_start, f_alpha;
  int64_t n_min;
};
template <class P>
static inline FireParams fire_params(const P& p) {
  return {p.fmax, p.dt_max, p.max_step, p.f_inc, p.f_dec, p.alpha_start, p.f_alpha, p.n_min};
}
static inline RelaxConst relax_const(const FireParams& f, int n3, double f_scale) {
  return {n3, f_scale, f.fmax, f.dt_max, f.max_step, f.f_inc, f.f_dec, f.alpha_start, f.f_alpha, f.n_min};
}

// the per-replica FIRE state dt | alpha | n_pos | n_taken, B words each: in device memory (carve), or the caller's arrays
struct FireState {
  double *dt, *alpha;
  int64_t *n_pos, *n_taken;
  double* carve(double* p, int64_t B) {  // takes 4 B words from p; returns the end
    *this = {p, p + B, (int64_t*)(p + 2 * B), (int64_t*)(p + 3 * B)};
    return p + 4 * B;
  }
  // device <- host (to_host = false) or host <- device, queued on st
  hipError_t copy(const FireState& host, int64_t B, bool to_host, hipStream_t st) const {
    void* d[4] = {dt, alpha, n_pos, n_taken};
    void* h[4] = {host.dt, host.alpha, host.n_pos, host.n_taken};
    for (int i = 0; i < 4; ++i) {
      const hipError_t e = to_host ? hipMemcpyAsync(h[i], d[i], (size_t)B * 8, hipMemcpyDeviceToHost, st)
                                   : hipMemcpyAsync(d[i], h[i], (size_t)B * 8, hipMemcpyHostToDevice, st);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
};

// argument checks of the three entries behind their own test of params (fn: the entry's name, the prefix of every message);
// ctx may be NULL (the message then goes where gdml_ctx_create's goes)
static inline int relax_check(gdml_ctx* ctx, const char* fn, int64_t B, int N, double f_scale, const double* lat,
                              const double* lat_inv, const FireParams& p, const double* R, const double* V, const FireState& s,
                              int64_t max_steps, int64_t record_every, const double* R_rec, const double* E_hist,
                              const double* fmax_hist, const double* E_end, const double* F_end, const int64_t* status) {
  if (max_steps < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: max_steps < 0", fn);
  if (record_every < 0 || (R_rec && record_every < 1))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: record_every < 0, or < 1 with R_rec", fn);
  GDML_TRY(traj_check_shape(ctx, fn, B, N));
  GDML_TRY(traj_check_f_scale(ctx, fn, f_scale));
  if (!(p.fmax > 0.0) || !isfinite(p.fmax)) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: fmax must be positive and finite", fn);
  if (!(p.max_step > 0.0) || !isfinite(p.max_step))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: max_step must be positive and finite", fn);
  if (!(p.f_inc >= 1.0) || !isfinite(p.f_inc)) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: f_inc < 1", fn);
  if (!(p.f_dec > 0.0 && p.f_dec < 1.0)) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: f_dec outside (0, 1)", fn);
  if (!(p.alpha_start > 0.0 && p.alpha_start <= 1.0))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: alpha_start outside (0, 1]", fn);
  if (!(p.f_alpha > 0.0 && p.f_alpha <= 1.0)) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: f_alpha outside (0, 1]", fn);
  if (p.n_min < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: n_min < 0", fn);
  GDML_TRY(traj_check_lattice(ctx, fn, lat, lat_inv));
  if (!R || !V || !s.dt || !s.alpha || !s.n_pos || !s.n_taken)
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: a state array (R, V, dt, alpha, n_pos, n_taken) is NULL", fn);
  if (!E_hist || !fmax_hist || !E_end || !F_end || !status)
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: an output array (E_hist, fmax_hist, E_end, F_end, status) is NULL", fn);
  if (!(p.dt_max > 0.0) || !isfinite(p.dt_max))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: dt_max must be positive and finite", fn);
  for (int64_t b = 0; b < B; ++b) {
    if (!(s.dt[b] > 0.0) || !isfinite(s.dt[b]))
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: dt of replica %lld must be positive and finite", fn, (long long)b);
    if (p.dt_max < s.dt[b])
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: dt_max is below dt of replica %lld", fn, (long long)b);
  }
  return GDML_OK;
}

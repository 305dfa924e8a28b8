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
// Sums: per-thread partial sums in index order, then the 256-slot tree (block_tree_sum, traj.h).  Two routes, ONE update function
// (relax_finish) on both:
//   general:       gdml_predict_dev for all B geometries into scratch (frozen replicas' results are discarded), then
//                  relax_update_kernel, one workgroup per replica
//   single launch: relax_step_kernel (D <= 256, B <= 8), the predictor's share being fused_core.h's, as in md_step_kernel;
//                  r(t+1) into the other half of a ping-pong buffer
// The host synchronises once per chunk and reads the status words; it stops when no replica is active.  Checks, prelude
// and the recorder of R_rec are traj.h's, shared with md.hip and pimd.hip.
// ------------------------------------------------------------------------------------------
#include <math.h>

#include "common.h"
#include "fused_core.h"
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
  FusedModel M;
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
  __shared__ double s_r[FUSED_MAX_N3], s_f[FUSED_MAX_N3];
  __shared__ double red[4][256];
  __shared__ double s_Eq;
  __shared__ unsigned s_ticket;
  const int tid = threadIdx.x;
  const int N = A.M.N, n3 = 3 * N;
  const int q = (int)blockIdx.y;
  if (A.S.status[2 * q] >= 0) return;
  if (tid < n3) s_r[tid] = A.inR[(int64_t)q * n3 + tid];
  __syncthreads();

  if (!fused_partials<KPL>(A.M, (const double*)s_r, s_fx, s_E, s_ticket)) return;
  double* fxs = &s_fx[0][0];
  fused_sum_partials(A.M, fxs, [&](double e) { s_Eq = e; });
  fused_jacobian(A.M, (const double*)s_r, s_g);
  __syncthreads();
  if (tid < n3) s_f[tid] = fused_force(N, s_g, fxs, tid);
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
  GDML_TRY(traj_check_shape(ctx, "gdml_relax_run", p->B, p->N));
  GDML_TRY(traj_check_f_scale(ctx, "gdml_relax_run", p->f_scale));
  if (!(p->fmax > 0.0) || !isfinite(p->fmax)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: fmax must be positive and finite");
  if (!(p->max_step > 0.0) || !isfinite(p->max_step))
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: max_step must be positive and finite");
  if (!(p->f_inc >= 1.0) || !isfinite(p->f_inc)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: f_inc < 1");
  if (!(p->f_dec > 0.0 && p->f_dec < 1.0)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: f_dec outside (0, 1)");
  if (!(p->alpha_start > 0.0 && p->alpha_start <= 1.0))
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: alpha_start outside (0, 1]");
  if (!(p->f_alpha > 0.0 && p->f_alpha <= 1.0)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: f_alpha outside (0, 1]");
  if (p->n_min < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_relax_run: n_min < 0");
  GDML_TRY(traj_check_lattice(ctx, "gdml_relax_run", p->lat, p->lat_inv));
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
  bool run;
  GDML_TRY(traj_prelude(ctx, "gdml_relax_run", p->N, p->B, first_bad_step, &run));
  if (!run) return GDML_OK;
  Model& md = ctx->model;
  const int64_t B = p->B;
  const int n3 = 3 * p->N;
  const int64_t nc = B * n3;
  const int64_t n_eval_max = max_steps + 1;
  // evaluations per chunk, and frames of R per chunk where they are recorded
  int64_t chunk_steps = (int64_t)ctx_opt(ctx, "predict.relax_chunk_steps", 32.0);
  if (chunk_steps < 1) chunk_steps = 1;
  if (chunk_steps > n_eval_max) chunk_steps = n_eval_max;
  Recorder rec;
  const int f_R = rec.add(R_rec, nc);
  rec.size(ctx, chunk_steps);

  const bool fused =
      fused_serves(md, B) && n3 <= FUSED_MAX_N3 && !ctx->profiling && ctx_opt_i(ctx, "predict.relax_fused", 1) != 0;
  const FusedPlan plan = fused_plan(ctx, md);

  // one allocation: two halves of R (the general route works in the first) | V | F | F', E' of the general route's prediction
  // | E | dt | alpha | n_pos | n_taken | status | bad | a chunk of the history (E, f_atom) and of frames | partials, tickets
  const int64_t n_state = 4 * nc + (fused ? 0 : nc + B) + 8 * B;
  const int64_t n_chunk = 2 * chunk_steps * B + rec.len();
  const int64_t n_part = fused ? fused_part_len(md, plan, B) + FUSED_MAX_Q : 0;
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
  double* d_part = rec.carve(c_fat + chunk_steps * B);
  unsigned* d_counter = (unsigned*)(d_part + fused_part_len(md, plan, B));

  hipStream_t st = ctx->stream;
  DROP_HIP(hipMemcpyAsync(half[0], R, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_V, V, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_dt, dt, (size_t)B * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_alpha, alpha, (size_t)B * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_npos, n_pos, (size_t)B * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_ntaken, n_taken, (size_t)B * 8, hipMemcpyHostToDevice, st));
  traj_fill_i64_kernel<<<ceil_div(3 * B, 256), 256, 0, st>>>(d_status, 3 * B, -1);  // status and bad
  if (fused) DROP_HIP(hipMemsetAsync(d_counter, 0, FUSED_MAX_Q * 8, st));
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
    fused_fill(A.M, md, plan, p->lat, p->lat_inv, d_part, d_counter);
    A.C = C; A.S = S;
  }

  // status (B,2), bad (B) and the chunk's history lie side by side: ONE copy per chunk brings them to the host
  const int64_t n_out = 3 * B + 2 * chunk_steps * B;
  std::vector<int64_t> h_out((size_t)n_out, -1);
  const int64_t* h_flags = h_out.data();
  const double* h_E = (const double*)(h_out.data() + 3 * B);
  const double* h_fat = h_E + chunk_steps * B;
  int64_t t = 0;
  bool active = true, any_bad = false;
  while (t <= max_steps && active && !any_bad) {
    const int64_t t0 = t;
    int64_t in_chunk = 0;
    for (; t <= max_steps && t - t0 < chunk_steps; ++t) {
      const bool on = R_rec && t % record_every == 0;
      if (on && in_chunk == rec.frames) break;
      RelaxSlot sl = {c_E + (t - t0) * B, c_fat + (t - t0) * B, on ? rec.slot(f_R, in_chunk) : nullptr};
      if (on) ++in_chunk;
      const int last = t == max_steps;
      if (fused) {
        A.sl = sl; A.t = t; A.last = last;
        A.inR = half[cur]; A.outR = half[cur ^ 1];
        fused_launch(plan, B, st, relax_step_kernel<1>, relax_step_kernel<2>, relax_step_kernel<4>, A);
        cur ^= 1;
      } else {
        // the timer of the previous evaluation's prediction is dropped unread: reading it would wait for it on the host
        ctx->phase_pending.clear();
        DROP_TRY(gdml_predict_dev(ctx, half[0], B, p->lat, p->lat_inv, d_Et, d_Ft));
        relax_update_kernel<<<(unsigned)B, 256, 0, st>>>(C, S, sl, half[0], d_Ft, d_Et, t, last);
      }
    }
    DROP_HIP(hipGetLastError());
    if (in_chunk > 0) DROP_HIP(rec.flush(st, in_chunk));
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

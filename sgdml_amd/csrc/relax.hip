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
// (relax_finish, relax_finish.h: gdml_neb_run calls it as well, on a whole band) on both:
//   general:       gdml_predict_dev for all B geometries into scratch (frozen replicas' results are discarded), then
//                  relax_update_kernel, one workgroup per replica
//   single launch: relax_step_kernel (D <= 256, B <= 8), the predictor's share being fused_core.h's, as in md_step_kernel;
//                  r(t+1) into the other half of a ping-pong buffer
// The host synchronises once per chunk and reads the status words; it stops when no replica is active.  Prelude, the recorder
// of R_rec and the chunk loop (traj_run_until_frozen) are traj.h's; the argument checks lie next to relax_finish.
// ------------------------------------------------------------------------------------------
#include <math.h>

#include "common.h"
#include "fused_core.h"
#include "traj.h"
#include "relax_finish.h"

// general route, one workgroup per replica: F', E' of all B geometries lie in Ft, Et (gdml_predict_dev); a frozen replica's
// are ignored
__global__ void __launch_bounds__(256) relax_update_kernel(RelaxConst C, RelaxState S, RelaxSlot sl, double* R, const double* Ft,
                                                           const double* Et, int64_t t, int last) {
  __shared__ double red[4][256];
  const int64_t q = blockIdx.x;
  if (S.status[2 * q] >= 0) return;
  double* r = R + q * C.n3;
  relax_finish(C, S, sl, q, t, last, r, Ft + q * C.n3, Et[q], r, nullptr, red, C.n3, q * C.n3);
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
  relax_finish(A.C, A.S, A.sl, q, A.t, A.last, s_r, s_f, s_Eq, out, out, red, A.C.n3, (int64_t)q * A.C.n3);
  if (tid == 0) A.M.counter[q] = 0u;  // the next launch on the stream finds it reset
}

extern "C" int gdml_relax_run(gdml_ctx* ctx, const gdml_relax_params* p, double* R, double* V, double* dt, double* alpha,
                              int64_t* n_pos, int64_t* n_taken, int64_t max_steps, int64_t record_every, double* R_rec,
                              double* E_hist, double* fmax_hist, double* E_end, double* F_end, int64_t* status,
                              int64_t* first_bad_step) {
  const char* fn = "gdml_relax_run";
  if (!p) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: params is NULL", fn);
  const FireParams fire = fire_params(*p);
  const FireState h_fire = {dt, alpha, n_pos, n_taken};
  GDML_TRY(relax_check(ctx, fn, p->B, p->N, p->f_scale, p->lat, p->lat_inv, fire, R, V, h_fire, max_steps, record_every, R_rec,
                       E_hist, fmax_hist, E_end, F_end, status));
  bool run;
  GDML_TRY(traj_prelude(ctx, fn, p->N, p->B, first_bad_step, &run));
  if (!run) return GDML_OK;
  Model& md = ctx->model;
  const int64_t B = p->B;
  const int n3 = 3 * p->N;
  const int64_t nc = B * n3;
  // evaluations per chunk, and frames of R per chunk where they are recorded
  FrozenRun fr = {B, max_steps, record_every, traj_frozen_chunk_steps(ctx, max_steps), 2, {E_hist, fmax_hist}};
  Recorder rec;
  const int f_R = rec.add(R_rec, nc);
  rec.size(ctx, fr.chunk_steps);

  const bool fused =
      fused_serves(md, B) && n3 <= FUSED_MAX_N3 && !ctx->profiling && ctx_opt_i(ctx, "predict.relax_fused", 1) != 0;
  const FusedPlan plan = fused_plan(ctx, md);

  // one allocation: two halves of R (the general route works in the first) | V | F | F', E' of the general route's prediction
  // | E | dt, alpha, n_pos, n_taken | status, bad, a chunk of the history (E, f_atom) | a chunk of frames | partials, tickets
  const int64_t n_state = 4 * nc + (fused ? 0 : nc + B) + 5 * B;
  const int64_t n_part = fused ? fused_part_len(md, plan, B) + FUSED_MAX_Q : 0;
  double* buf = nullptr;
  GDML_TRY(ctx_alloc(ctx, (void**)&buf, (n_state + fr.words() + rec.len() + n_part) * 8));
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
  FireState d_fire;
  double* d_part = rec.carve(fr.carve(d_fire.carve(d_E + B, B)));
  unsigned* d_counter = (unsigned*)(d_part + fused_part_len(md, plan, B));

  hipStream_t st = ctx->stream;
  DROP_HIP(hipMemcpyAsync(half[0], R, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_V, V, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(d_fire.copy(h_fire, B, false, st));
  if (fused) DROP_HIP(hipMemsetAsync(d_counter, 0, FUSED_MAX_Q * 8, st));
  // the caller's arrays are pageable: the copies above have to be through before they may change
  DROP_HIP(hipStreamSynchronize(st));

  const RelaxConst C = relax_const(fire, n3, p->f_scale);
  RelaxState S = {d_V, d_F, d_E, d_fire.dt, d_fire.alpha, d_fire.n_pos, d_fire.n_taken, fr.status(), fr.bad()};

  RelaxStepArgs A;
  memset(&A, 0, sizeof(A));
  if (fused) {
    fused_fill(A.M, md, plan, p->lat, p->lat_inv, d_part, d_counter);
    A.C = C; A.S = S;
  }

  DROP_TRY(traj_run_until_frozen(ctx, rec, R_rec != nullptr, fr, [&](int64_t te, int64_t row, int64_t frame, int last) {
    RelaxSlot sl = {fr.row(0, row), fr.row(1, row), frame >= 0 ? rec.slot(f_R, frame) : nullptr};
    if (fused) {
      A.sl = sl; A.t = te; A.last = last;
      A.inR = half[cur]; A.outR = half[cur ^ 1];
      fused_launch(plan, B, st, relax_step_kernel<1>, relax_step_kernel<2>, relax_step_kernel<4>, A);
      cur ^= 1;
    } else {
      // the timer of the previous evaluation's prediction is dropped unread: reading it would wait for it on the host
      ctx->phase_pending.clear();
      GDML_TRY(gdml_predict_dev(ctx, half[0], B, p->lat, p->lat_inv, d_Et, d_Ft));
      relax_update_kernel<<<(unsigned)B, 256, 0, st>>>(C, S, sl, half[0], d_Ft, d_Et, te, last);
    }
    return (int)GDML_OK;
  }));
  DROP_HIP(hipMemcpyAsync(R, half[cur], (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(V, d_V, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(F_end, d_F, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(E_end, d_E, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(d_fire.copy(h_fire, B, true, st));
  DROP_HIP(hipStreamSynchronize(st));
  // a frozen replica repeats its last history values and its end positions up to the last evaluation made
  const TrajFrames frames = {R_rec, R, n3};
  fr.finish(status, first_bad_step, &frames, 1);
  return drop(GDML_OK);
}

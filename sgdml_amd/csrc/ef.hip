// ------------------------------------------------------------------------------------------
// Eigenvector following (gdml_ef_run): a search for minima and first-order saddles in the Hessian's eigenbasis.  Every
// evaluation runs the spectrum of vib.hip as it is (spectrum_slice: Hessian, projection, eigensolver, finish) with unit masses
// and h_scale = f_scale, and adds ONE kernel, ef_step_kernel: the step in the eigenbasis, the trust radius, the mode tracking
// and the per-geometry convergence (the contract: include/gdml_hip.h; tests/_ef_ref.py states the same).  Its driver is
// gdml_relax_run's general route: plain launches queued back to back, traj.h's chunk loop, one synchronisation per chunk.
// ------------------------------------------------------------------------------------------
#include <math.h>

#include "vib.h"

namespace {

struct EfConst {
  int n3, order, has_t;
  double f_scale, fmax, trust_min, trust_max;
};
struct EfState {  // per geometry, in device memory: the optimiser's state, the end-of-run outputs and status
  double *R, *tvec, *trust, *E_prev, *dE_pred;
  int64_t* flags;   // bit 0: a previous step exists, bit 1: that step was clipped
  double *F, *E, *w, *mode;
  int64_t *n_rigid, *n_neg;
  int64_t* status;  // (B,2) as gdml_relax_run's
  int64_t* bad;
};
struct EfEval {  // this evaluation's results for one slice of geometries
  const double *V, *w, *Ft, *Et;  // eigenvectors as rows (bc,n3,n3), spectrum after vib_finish_kernel (bc,n3), F', E'
  const int64_t *sweeps, *n_rigid, *n_neg;
};
struct EfSlot {  // where this evaluation goes in the chunk buffers
  double *E, *fat;  // (B) rows of the history
  double* wf;       // (B) row: eigenvalue of the followed mode
  int64_t* kf;      // (B) row: its index
  double* R;        // (B,3N) frame; null when this is no recording evaluation
};

// dynamic LDS: g [n3] | gt [n3] | s [n3] (the overlaps v_i . t until the followed mode is chosen) | red [256] | followed index
// (no static LDS beside it: statics precede the dynamic region and would shift its base off the doubles' alignment)
static inline size_t ef_step_lds(int n3) { return (size_t)(3 * n3 + 256 + 1) * 8; }

// One evaluation of geometry b0 + blockIdx.x once its F', E', spectrum and eigenvectors are known.  One workgroup per geometry;
// it writes nothing another workgroup reads.  Sums over modes: per-thread partial sums in index order, then the 256-slot tree;
// row . vector products: one wavefront per row, lanes stride the columns, the xor butterfly; the back-projection sums over the
// modes in ascending order, one coordinate per thread.
__global__ void __launch_bounds__(256) ef_step_kernel(EfConst C, EfState S, EfEval Ev, EfSlot sl, int64_t b0, int64_t t,
                                                      int last) {
  extern __shared__ __attribute__((aligned(8))) unsigned char ef_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n3 = C.n3;
  const int64_t ql = blockIdx.x, q = b0 + ql;
  if (S.status[2 * q] >= 0) return;  // frozen by an earlier launch: never written again
  double* g = reinterpret_cast<double*>(ef_raw);
  double* gt = g + n3;
  double* s = gt + n3;
  double (*red)[256] = reinterpret_cast<double (*)[256]>(s + n3);
  int* s_k = reinterpret_cast<int*>(s + n3 + 256);
  const int64_t o = q * n3;
  double* r = S.R + o;
  double* tv = C.has_t ? S.tvec + o : nullptr;
  const double* fp = Ev.Ft + ql * n3;
  const double* wq = Ev.w + ql * n3;
  const double* Vq = Ev.V + ql * n3 * (int64_t)n3;
  const double e = Ev.Et[ql];
  const int n_rigid = (int)Ev.n_rigid[ql], nv = n3 - n_rigid;

  // a. gradient, finiteness, this evaluation's outputs
  int nf = 0;
  for (int k = tid; k < n3; k += 256) {
    const double f = fp[k], wk = wq[k];
    g[k] = -C.f_scale * f;
    nf |= !(isfinite(r[k]) && isfinite(f) && isfinite(wk));
    S.F[o + k] = f;
    S.w[o + k] = wk;
    if (sl.R) sl.R[o + k] = r[k];
  }
  nf = __syncthreads_or(nf);
  double fa = 0.0;
  for (int a = tid; 3 * a < n3; a += 256) {
    const double g0 = g[3 * a], g1 = g[3 * a + 1], g2 = g[3 * a + 2];
    const double nrm = sqrt(g0 * g0 + g1 * g1 + g2 * g2);
    fa = nrm > fa ? nrm : fa;
  }
  red[0][tid] = fa;
  __syncthreads();
  block_tree_sum<0, 1>(red, tid);
  const double f_atom = red[0][0];  // (the maximum skips a NaN)
  __syncthreads();
  const bool bad_now = nf || !isfinite(e) || Ev.sweeps[ql] > SYM_EIG_MAX_SWEEPS;

  // c. gradient in the eigenbasis, and the overlaps with the follow vector
  for (int i = wave; i < nv; i += 4) {
    const double* v = Vq + (int64_t)i * n3;
    double ag = 0.0, at = 0.0;
    for (int j = lane; j < n3; j += 64) {
      const double vj = v[j];
      ag += vj * g[j];
      if (tv) at += vj * tv[j];
    }
    ag = wave_sum(ag);
    at = wave_sum(at);
    if (lane == 0) { gt[i] = ag; s[i] = at; }
  }
  __syncthreads();
  // d. the followed mode: the largest |v_i . t|, the lowest index on ties
  if (tid == 0) {
    int k = 0;
    if (C.order == 1 && tv) {
      double best = -1.0;
      for (int i = 0; i < nv; ++i) {
        const double a = fabs(s[i]);
        if (a > best) { best = a; k = i; }
      }
    }
    *s_k = k;
  }
  __syncthreads();
  const int kfol = *s_k;
  for (int j = tid; j < n3; j += 256) S.mode[o + j] = C.order == 1 ? Vq[(int64_t)kfol * n3 + j] : 0.0;
  if (tid == 0) {
    S.E[q] = e;
    S.n_rigid[q] = n_rigid;
    S.n_neg[q] = Ev.n_neg[ql];
    sl.wf[q] = nv > 0 ? wq[kfol] : 0.0;
    sl.kf[q] = kfol;
    sl.E[q] = e;
    sl.fat[q] = f_atom;
    if (bad_now && S.bad[q] < 0) S.bad[q] = t;
  }
  const bool conv = !bad_now && f_atom < C.fmax;
  if (conv || last) {  // frozen from here on: the state stays what this evaluation found
    if (tid == 0) {
      S.status[2 * q] = conv ? 1 : 0;
      S.status[2 * q + 1] = t;
    }
    return;
  }

  // b. trust radius from the last step's predicted and actual change of the energy
  double trust = S.trust[q];
  const int64_t fl = S.flags[q];
  if (fl & 1) {
    const double dEp = S.dE_pred[q], Ep = S.E_prev[q];
    if (fabs(dEp) > 1e-8 * fmax(fabs(e), fabs(Ep)) * C.f_scale) {
      const double rho = C.f_scale * (e - Ep) / dEp;
      if (rho < 0.25 || rho > 1.75) trust = fmax(0.5 * trust, C.trust_min);
      else if (rho > 0.75 && rho < 1.25 && (fl & 2)) trust = fmin(2.0 * trust, C.trust_max);
    }
  }
  // e. the rational-function step of every mode in closed form
  double p2 = 0.0;
  for (int i = tid; i < nv; i += 256) {
    const double wi = wq[i], gi = gt[i];
    const double d = fabs(wi) + sqrt(wi * wi + 4.0 * (gi * gi));
    double si = d > 0.0 ? -2.0 * gi / d : 0.0;
    if (C.order == 1 && i == kfol) si = -si;
    s[i] = si;
    p2 += si * si;
  }
  // f. trust radius
  const double s_nrm = sqrt(vib_sum(red, tid, p2));
  const bool clip = s_nrm > trust;
  const double scale = trust / s_nrm;
  // g. predicted change, new positions, follow vector
  double pe = 0.0;
  for (int i = tid; i < nv; i += 256) {
    double si = s[i];
    if (clip) si = si * scale;
    s[i] = si;
    pe += gt[i] * si + 0.5 * wq[i] * (si * si);
  }
  const double dE = vib_sum(red, tid, pe);
  for (int j = tid; j < n3; j += 256) {
    double acc = 0.0;
    for (int i = 0; i < nv; ++i) acc += s[i] * Vq[(int64_t)i * n3 + j];
    r[j] = r[j] + acc;
    if (tv && C.order == 1) tv[j] = Vq[(int64_t)kfol * n3 + j];
  }
  if (tid == 0) {
    S.trust[q] = trust;
    S.E_prev[q] = e;
    S.dE_pred[q] = dE;
    S.flags[q] = 1 | (clip ? 2 : 0);
  }
}

int ef_check(gdml_ctx* ctx, const gdml_ef_params* p, const double* R, const double* trust, const double* E_prev,
             const double* dE_pred, const int64_t* flags, const double* t, int64_t max_steps, int64_t record_every,
             const double* R_rec, const void* const* out, int n_out) {
  const char* fn = "gdml_ef_run";
  if (!p) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: params is NULL", fn);
  if (max_steps < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: max_steps < 0", fn);
  if (record_every < 0 || (R_rec && record_every < 1))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: record_every < 0, or < 1 with R_rec", fn);
  GDML_TRY(traj_check_shape(ctx, fn, p->B, p->N));
  if (!isfinite(p->f_scale) || !(p->f_scale > 0.0))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: f_scale must be positive and finite", fn);
  if (!(p->fmax > 0.0) || !isfinite(p->fmax)) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: fmax must be positive and finite", fn);
  if (p->order != 0 && p->order != 1) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: order must be 0 (minimum) or 1 (saddle)", fn);
  if (!(p->trust_min > 0.0) || !isfinite(p->trust_min))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: trust_min must be positive and finite", fn);
  if (!(p->trust_max >= p->trust_min) || !isfinite(p->trust_max))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: trust_max must be finite and at least trust_min", fn);
  GDML_TRY(spectrum_check_projection(ctx, fn, p->project, p->lat, p->lat_inv));
  if (t && p->order == 0) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: a follow vector with order = 0", fn);
  if (!R || !trust || !E_prev || !dE_pred || !flags)
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: a state array (R, trust, E_prev, dE_pred, flags) is NULL", fn);
  for (int i = 0; i < n_out; ++i)
    if (!out[i])
      return gdml_fail(ctx, GDML_ERR_INVALID,
                       "%s: an output array (E_hist, fmax_hist, w_follow_hist, E_end, F_end, w_end, n_rigid, n_neg, mode_end, "
                       "status) is NULL", fn);
  GDML_TRY(spectrum_check_atoms(ctx, fn, p->N));
  for (int64_t b = 0; b < p->B; ++b) {
    if (!(trust[b] >= p->trust_min && trust[b] <= p->trust_max))
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: trust of geometry %lld outside [trust_min, trust_max]", fn, (long long)b);
    if (flags[b] < 0 || flags[b] > 3) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: flags of geometry %lld outside 0 .. 3", fn, (long long)b);
    if ((flags[b] & 1) && !(isfinite(E_prev[b]) && isfinite(dE_pred[b])))
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: E_prev or dE_pred of geometry %lld is not finite", fn, (long long)b);
  }
  return spectrum_check_finite(ctx, fn, p->N, p->B, R, t);
}

}  // namespace

extern "C" int gdml_ef_run(gdml_ctx* ctx, const gdml_ef_params* p, double* R, double* trust, double* E_prev, double* dE_pred,
                           int64_t* flags, double* t_follow, int64_t max_steps, int64_t record_every, double* R_rec,
                           double* E_hist, double* fmax_hist, double* w_follow_hist, int64_t* k_follow_hist, double* E_end,
                           double* F_end, double* w_end, int64_t* n_rigid, int64_t* n_neg, double* mode_end, int64_t* status,
                           int64_t* first_bad_step) {
  const void* outs[] = {E_hist, fmax_hist, w_follow_hist, E_end, F_end, w_end, n_rigid, n_neg, mode_end, status};
  GDML_TRY(ef_check(ctx, p, R, trust, E_prev, dE_pred, flags, t_follow, max_steps, record_every, R_rec, outs, 10));
  bool run;
  GDML_TRY(traj_prelude(ctx, "gdml_ef_run", p->N, p->B, first_bad_step, &run));
  if (!run) return GDML_OK;
  const int64_t B = p->B;
  const int N = p->N, n3 = 3 * N;
  const int64_t nc = B * n3;
  // evaluations per chunk, and frames of R per chunk where they are recorded: gdml_relax_run's
  FrozenRun fr = {B, max_steps, record_every, traj_frozen_chunk_steps(ctx, max_steps), 4,
                  {E_hist, fmax_hist, w_follow_hist, k_follow_hist}};
  Recorder rec;
  const int f_R = rec.add(R_rec, nc);
  rec.size(ctx, fr.chunk_steps);
  // geometries per slice of an evaluation: gdml_vib_run's chunk
  const int64_t slice = spectrum_slice_len(ctx->num_cus, B, n3, (int64_t)ctx_opt(ctx, "predict.vib_chunk", 0.0));
  const SymEigPlan plan = sym_eig_plan(ctx->num_cus, slice, n3, true);

  // one carve.  Per slice: the spectrum's workspace without R (SpectrumWs; F', E' and unit masses in its F, E and mass).
  // Per run: R | t | F_end | w_end | mode_end | E_end | trust | E_prev | dE_pred | flags, n_rigid, n_neg | status, bad, a chunk of
  // the history (E, f_atom, w_follow, k_follow) | a chunk of frames
  const SpectrumWs ws = spectrum_ws(slice, N, plan.work_doubles, false);
  const int64_t n_run = 5 * nc + 7 * B + fr.words() + rec.len();
  double* buf;
  GDML_TRY(ctx_slot(ctx, SLOT_EF_WS, (ws.total + n_run) * 8, &buf));
  const Spectrum Sp = spectrum_carve(buf, ws);
  const SpectrumIn in = {N, p->project, p->f_scale, p->lat, p->lat_inv};
  EfState S;
  S.R = buf + ws.total;
  S.tvec = S.R + nc;
  S.F = S.tvec + nc;
  S.w = S.F + nc;
  S.mode = S.w + nc;
  S.E = S.mode + nc;
  S.trust = S.E + B;
  S.E_prev = S.trust + B;
  S.dE_pred = S.E_prev + B;
  S.flags = (int64_t*)(S.dE_pred + B);
  S.n_rigid = S.flags + B;
  S.n_neg = S.n_rigid + B;
  rec.carve(fr.carve((double*)(S.n_neg + B)));
  S.status = fr.status();
  S.bad = fr.bad();

  hipStream_t st = ctx->stream;
  const std::vector<double> ones((size_t)N, 1.0);
  HIP_CHECK(ctx, hipMemcpyAsync(Sp.mass, ones.data(), (size_t)N * 8, hipMemcpyHostToDevice, st));
  HIP_CHECK(ctx, hipMemcpyAsync(S.R, R, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  if (t_follow) HIP_CHECK(ctx, hipMemcpyAsync(S.tvec, t_follow, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  HIP_CHECK(ctx, hipMemcpyAsync(S.trust, trust, (size_t)B * 8, hipMemcpyHostToDevice, st));
  HIP_CHECK(ctx, hipMemcpyAsync(S.E_prev, E_prev, (size_t)B * 8, hipMemcpyHostToDevice, st));
  HIP_CHECK(ctx, hipMemcpyAsync(S.dE_pred, dE_pred, (size_t)B * 8, hipMemcpyHostToDevice, st));
  HIP_CHECK(ctx, hipMemcpyAsync(S.flags, flags, (size_t)B * 8, hipMemcpyHostToDevice, st));
  // the caller's arrays are pageable: the copies above have to be through before they may change
  HIP_CHECK(ctx, hipStreamSynchronize(st));

  EfConst C;
  C.n3 = n3; C.order = p->order; C.has_t = t_follow != nullptr;
  C.f_scale = p->f_scale; C.fmax = p->fmax; C.trust_min = p->trust_min; C.trust_max = p->trust_max;

  GDML_TRY(traj_run_until_frozen(ctx, rec, R_rec != nullptr, fr, [&](int64_t te, int64_t row, int64_t frame, int last) {
    const EfSlot sl = {fr.row(0, row), fr.row(1, row), fr.row(2, row), (int64_t*)fr.row(3, row),
                       frame >= 0 ? rec.slot(f_R, frame) : nullptr};
    // the timer of the previous Hessian is dropped unread: reading it would wait for it on the host
    ctx->phase_pending.clear();
    for (int64_t b0 = 0; b0 < B; b0 += slice) {
      const int64_t bc = B - b0 < slice ? B - b0 : slice;
      GDML_TRY(spectrum_slice(ctx, plan, Sp, in, S.R + b0 * n3, bc));
      const EfEval Ev = {Sp.H, Sp.w, Sp.F, Sp.E, Sp.sweeps, Sp.n_rigid, Sp.n_neg};
      hipLaunchKernelGGL(ef_step_kernel, dim3((unsigned)bc), dim3(256), ef_step_lds(n3), st, C, S, Ev, sl, b0, te, last);
      HIP_CHECK(ctx, hipGetLastError());
      ctx->launch_counter++;
    }
    return (int)GDML_OK;
  }));
  HIP_CHECK(ctx, hipMemcpyAsync(R, S.R, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  if (t_follow) HIP_CHECK(ctx, hipMemcpyAsync(t_follow, S.tvec, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(trust, S.trust, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(E_prev, S.E_prev, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(dE_pred, S.dE_pred, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(flags, S.flags, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(E_end, S.E, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(F_end, S.F, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(w_end, S.w, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(mode_end, S.mode, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(n_rigid, S.n_rigid, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(n_neg, S.n_neg, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipStreamSynchronize(st));
  // a frozen geometry repeats its last history values and its end positions up to the last evaluation made (the launches
  // behind its freeze wrote nothing for it)
  const TrajFrames frames = {R_rec, R, n3};
  fr.finish(status, first_bad_step, &frames, 1);
  return GDML_OK;
}

// ------------------------------------------------------------------------------------------
// Variable-cell relaxation (gdml_cell_relax_run): B independent periodic geometries relax atoms and cell by FIRE in the form
// ASE's FIRE(UnitCellFilter(atoms)) uses.  The contract (include/gdml_hip.h and tests/_cellrelax_ref.py state the same):
//   state per geometry: reference lattice L0 (fixed), u = (s_1 .. s_N, C) with C = cell_factor Fd, r_i = Fd s_i, L = Fd L0;
//   ONE FIRE system over the 3N + 9 coordinates of u (v, dt, alpha, n_pos, n_taken).  Evaluation t of an active geometry:
//   1. Fd = C / cell_factor; L = Fd L0; r = Fd s; Vol = |det L|        (cell_geometry below: fp64, no fused multiply-adds,
//      product sums left to right, inverses by the adjugate in the order the header writes down)
//   2. E', F', W' = gdml_predict_virial_cells_dev(r, L, L^-1) for all B geometries (frozen ones' results are discarded)
//   3. g = f_scale F';  G_i = Fd^T g_i;  T = mask o (f_scale W' + pressure Vol I);  G_cell = -T Fd^-T / cell_factor
//   4. relax_finish (relax_finish.h, unchanged) on u with G over n3 = 3N + 9: history, convergence, freezing, the FIRE update
// Per evaluation: the prediction's launches, then cell_update_kernel, one workgroup of 256 per geometry, which also writes
// the Cartesian r(t+1), L(t+1), L^-1(t+1) the next prediction reads.  cell_start_kernel makes those of the start.  There is no
// single-launch route: FusedModel (fused_core.h) holds one Lattice by value.  Prelude, recorder and chunk loop are traj.h's.
// ------------------------------------------------------------------------------------------
#include <math.h>

#include "common.h"
#include "traj.h"
#include "relax_finish.h"

struct Mat3 {
  double m[9];
};

// adjugate and determinant in the header's order; no fused multiply-adds (the host checks and the restatement use the same)
__host__ __device__ static inline double mat3_adj(const double* a, double* adj) {
#pragma clang fp contract(off)
  adj[0] = a[4] * a[8] - a[5] * a[7];
  adj[1] = a[2] * a[7] - a[1] * a[8];
  adj[2] = a[1] * a[5] - a[2] * a[4];
  adj[3] = a[5] * a[6] - a[3] * a[8];
  adj[4] = a[0] * a[8] - a[2] * a[6];
  adj[5] = a[2] * a[3] - a[0] * a[5];
  adj[6] = a[3] * a[7] - a[4] * a[6];
  adj[7] = a[1] * a[6] - a[0] * a[7];
  adj[8] = a[0] * a[4] - a[1] * a[3];
  return a[0] * adj[0] + a[1] * adj[3] + a[2] * adj[6];
}

struct CellGeom {
  Mat3 Fd, Fi, L, Li;  // deformation gradient, its inverse, lattice, its inverse
  double det;          // det L
};

// step 1 for one geometry: every thread of a workgroup computes the same values
__device__ __forceinline__ void cell_geometry(const double* C, const double* L0, double cell_factor, CellGeom& g) {
#pragma clang fp contract(off)
  for (int k = 0; k < 9; ++k) g.Fd.m[k] = C[k] / cell_factor;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b)
      g.L.m[3 * a + b] = g.Fd.m[3 * a] * L0[b] + g.Fd.m[3 * a + 1] * L0[3 + b] + g.Fd.m[3 * a + 2] * L0[6 + b];
  double adj[9];
  const double dF = mat3_adj(g.Fd.m, adj);
  for (int k = 0; k < 9; ++k) g.Fi.m[k] = adj[k] / dF;
  g.det = mat3_adj(g.L.m, adj);
  for (int k = 0; k < 9; ++k) g.Li.m[k] = adj[k] / g.det;
}

// r = Fd s for the geometry's N atoms, L and L^-1: what the next prediction reads
__device__ __forceinline__ void cell_write_cartesian(const CellGeom& g, const double* s, int n3a, double* r, double* L, double* Li) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  for (int k = tid; k < n3a; k += 256) {
    const int a = k / 3, c = k - 3 * a;
    r[k] = g.Fd.m[3 * c] * s[3 * a] + g.Fd.m[3 * c + 1] * s[3 * a + 1] + g.Fd.m[3 * c + 2] * s[3 * a + 2];
  }
  if (tid < 9) {
    L[tid] = g.L.m[tid];
    Li[tid] = g.Li.m[tid];
  }
}

struct CellConst {
  int n3a;  // 3N
  double f_scale, pressure, cell_factor;
  double mask[9];
};
struct CellArrays {  // device memory, per geometry
  double* U;         // (B,3N+9): s | C
  const double* L0;  // (B,9)
  double *R, *L, *Li;  // (B,3N), (B,9), (B,9): Cartesian positions, lattice and inverse of the current evaluation
  double* G;           // (B,3N+9): the generalised force of this evaluation
  const double *Ft, *Et, *Wt;  // F', E', W' of all B geometries
  double *F_end, *W_end, *vol_end;
};
struct CellSlot {  // where this evaluation goes in the chunk buffers beyond RelaxSlot's
  double* vol;       // (B) row of the volume history
  double *R, *lat;   // frame (B,3N), (B,9), or null
};

// before evaluation 0: r, L, L^-1 of the start
__global__ void __launch_bounds__(256) cell_start_kernel(CellConst K, CellArrays A, int n3) {
  const int64_t q = blockIdx.x;
  const double* u = A.U + q * n3;
  CellGeom g;
  cell_geometry(u + K.n3a, A.L0 + q * 9, K.cell_factor, g);
  cell_write_cartesian(g, u, K.n3a, A.R + q * K.n3a, A.L + q * 9, A.Li + q * 9);
}

// one workgroup per geometry, behind the prediction of evaluation t
__global__ void __launch_bounds__(256) cell_update_kernel(CellConst K, RelaxConst C, RelaxState S, RelaxSlot sl, CellSlot cs,
                                                          CellArrays A, int64_t t, int last) {
  __shared__ double red[4][256];
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  if (S.status[2 * q] >= 0) return;
  const int n3 = C.n3, n3a = K.n3a;
  double* u = A.U + q * n3;
  double* G = A.G + q * n3;
  const double* fp = A.Ft + q * n3a;
  const double* w = A.Wt + q * 9;
  CellGeom g;
  cell_geometry(u + n3a, A.L0 + q * 9, K.cell_factor, g);
  const double vol = fabs(g.det);
  const bool det_ok = isfinite(g.det) && g.det != 0.0;
  {
#pragma clang fp contract(off)
    for (int k = tid; k < n3a; k += 256) {  // G_i = Fd^T g_i
      const int a = k / 3, c = k - 3 * a;
      const double g0 = K.f_scale * fp[3 * a], g1 = K.f_scale * fp[3 * a + 1], g2 = K.f_scale * fp[3 * a + 2];
      G[k] = g.Fd.m[c] * g0 + g.Fd.m[3 + c] * g1 + g.Fd.m[6 + c] * g2;
      A.F_end[q * n3a + k] = fp[k];
      if (cs.R) cs.R[q * n3a + k] = A.R[q * n3a + k];
    }
    if (tid < 9) {  // G_cell = -T Fd^-T / cell_factor, (T Fd^-T)_ab = sum_c T_ac Fi_bc
      const int a = tid / 3, b = tid - 3 * a;
      double T[3];
      for (int c = 0; c < 3; ++c)
        T[c] = K.mask[3 * a + c] * (K.f_scale * w[3 * a + c] + (a == c ? K.pressure * vol : 0.0));
      const double x = T[0] * g.Fi.m[3 * b] + T[1] * g.Fi.m[3 * b + 1] + T[2] * g.Fi.m[3 * b + 2];
      G[n3a + tid] = det_ok ? -x / K.cell_factor : NAN;  // a zero or non-finite det L is a non-finite value of the geometry
      A.W_end[q * 9 + tid] = w[tid];
      if (cs.lat) cs.lat[q * 9 + tid] = g.L.m[tid];
    }
    if (tid == 0) {
      cs.vol[q] = vol;
      A.vol_end[q] = vol;
    }
  }
  __syncthreads();
  if (relax_finish(C, S, sl, q, t, last, u, G, A.Et[q], u, nullptr, red, n3, q * n3)) return;
  __syncthreads();  // u(t+1) is complete
  cell_geometry(u + n3a, A.L0 + q * 9, K.cell_factor, g);
  cell_write_cartesian(g, u, n3a, A.R + q * n3a, A.L + q * 9, A.Li + q * 9);
}

// |det| at most 1e-12 of the cube of the largest entry, or anything not finite (GDMLPredict's check_lattice)
static bool mat3_regular(const double* a) {
  double adj[9], big = 0.0;
  for (int k = 0; k < 9; ++k) {
    if (!isfinite(a[k])) return false;
    big = fmax(big, fabs(a[k]));
  }
  const double det = mat3_adj(a, adj);
  return isfinite(det) && fabs(det) > 1e-12 * big * big * big;
}

extern "C" int gdml_cell_relax_run(gdml_ctx* ctx, const gdml_cell_relax_params* p, double* Sr, double* Cc, const double* L0,
                                   double* V, double* dt, double* alpha, int64_t* n_pos, int64_t* n_taken, int64_t max_steps,
                                   int64_t record_every, double* R_rec, double* lat_rec, double* E_hist, double* vol_hist,
                                   double* fmax_hist, double* R_end, double* lat_end, double* E_end, double* F_end,
                                   double* W_end, double* vol_end, int64_t* status, int64_t* first_bad_step) {
  const char* fn = "gdml_cell_relax_run";
  if (!p) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: params is NULL", fn);
  const FireParams fire = fire_params(*p);
  const FireState h_fire = {dt, alpha, n_pos, n_taken};
  GDML_TRY(relax_check(ctx, fn, p->B, p->N, p->f_scale, nullptr, nullptr, fire, Sr, V, h_fire, max_steps, record_every,
                       R_rec ? R_rec : lat_rec, E_hist, fmax_hist, E_end, F_end, status));
  if (!L0) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: L0 is NULL (a cell relaxation needs a lattice per geometry)", fn);
  if (!Cc) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: Cc is NULL", fn);
  if (!vol_hist || !R_end || !lat_end || !W_end || !vol_end)
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: an output array (vol_hist, R_end, lat_end, W_end, vol_end) is NULL", fn);
  if (!(p->cell_factor > 0.0) || !isfinite(p->cell_factor))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: cell_factor must be positive and finite", fn);
  if (!isfinite(p->pressure)) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: pressure is not finite", fn);
  if (p->mask)
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        const double m = p->mask[3 * a + b];
        if ((m != 0.0 && m != 1.0) || m != p->mask[3 * b + a])
          return gdml_fail(ctx, GDML_ERR_INVALID, "%s: mask must be a symmetric 3 x 3 array of 0 and 1", fn);
      }
  for (int64_t b = 0; b < p->B; ++b) {
    if (!mat3_regular(L0 + 9 * b))
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: L0 of geometry %lld is singular or not finite", fn, (long long)b);
    if (!mat3_regular(Cc + 9 * b))
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: C of geometry %lld is singular or not finite", fn, (long long)b);
  }
  bool run;
  GDML_TRY(traj_prelude(ctx, fn, p->N, p->B, first_bad_step, &run));
  if (!run) return GDML_OK;
  const int64_t B = p->B;
  const int n3a = 3 * p->N, n3 = n3a + 9;
  const int64_t na = B * n3a, nu = B * n3;
  FrozenRun fr = {B, max_steps, record_every, traj_frozen_chunk_steps(ctx, max_steps), 3, {E_hist, fmax_hist, vol_hist}};
  Recorder rec;
  const int f_R = rec.add(R_rec, na);
  const int f_L = rec.add(lat_rec, 9 * B);
  rec.size(ctx, fr.chunk_steps);

  // one allocation: U | V | G | G kept | R | F' | F_end | L | L^-1 | L0 | W' | W_end | E' | vol_end | E | dt, alpha, n_pos,
  // n_taken | status, bad, a chunk of the history (E, f_atom, Vol) | a chunk of frames
  const int64_t n_state = 4 * nu + 3 * na + 5 * 9 * B + 7 * B;
  double* buf = nullptr;
  GDML_TRY(ctx_alloc(ctx, (void**)&buf, (n_state + fr.words() + rec.len()) * 8));
  auto drop = [&](int rc) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)ctx_free(ctx, buf);
    return rc;
  };
  double* d_U = buf;
  double* d_V = d_U + nu;
  double* d_G = d_V + nu;
  double* d_Gk = d_G + nu;
  double* d_R = d_Gk + nu;
  double* d_Ft = d_R + na;
  double* d_Fe = d_Ft + na;
  double* d_L = d_Fe + na;
  double* d_Li = d_L + 9 * B;
  double* d_L0 = d_Li + 9 * B;
  double* d_Wt = d_L0 + 9 * B;
  double* d_We = d_Wt + 9 * B;
  double* d_Et = d_We + 9 * B;
  double* d_ve = d_Et + B;
  double* d_E = d_ve + B;
  FireState d_fire;
  rec.carve(fr.carve(d_fire.carve(d_E + B, B)));

  hipStream_t st = ctx->stream;
  DROP_HIP(hipMemcpy2DAsync(d_U, (size_t)n3 * 8, Sr, (size_t)n3a * 8, (size_t)n3a * 8, (size_t)B, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpy2DAsync(d_U + n3a, (size_t)n3 * 8, Cc, 72, 72, (size_t)B, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_L0, L0, (size_t)B * 72, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(d_V, V, (size_t)nu * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(d_fire.copy(h_fire, B, false, st));
  // the caller's arrays are pageable: the copies above have to be through before they may change
  DROP_HIP(hipStreamSynchronize(st));

  const RelaxConst C = relax_const(fire, n3, 1.0);  // G is in the caller's units already
  RelaxState S = {d_V, d_Gk, d_E, d_fire.dt, d_fire.alpha, d_fire.n_pos, d_fire.n_taken, fr.status(), fr.bad()};
  CellConst K;
  K.n3a = n3a;
  K.f_scale = p->f_scale;
  K.pressure = p->pressure;
  K.cell_factor = p->cell_factor;
  for (int k = 0; k < 9; ++k) K.mask[k] = p->mask ? p->mask[k] : 1.0;
  CellArrays A = {d_U, d_L0, d_R, d_L, d_Li, d_G, d_Ft, d_Et, d_Wt, d_Fe, d_We, d_ve};

  cell_start_kernel<<<(unsigned)B, 256, 0, st>>>(K, A, n3);

  DROP_TRY(traj_run_until_frozen(ctx, rec, R_rec != nullptr || lat_rec != nullptr, fr,
                                 [&](int64_t te, int64_t row, int64_t frame, int last) {
    RelaxSlot sl = {fr.row(0, row), fr.row(1, row), nullptr};
    CellSlot cs = {fr.row(2, row), frame >= 0 ? rec.slot(f_R, frame) : nullptr, frame >= 0 ? rec.slot(f_L, frame) : nullptr};
    // the timer of the previous evaluation's prediction is dropped unread: reading it would wait for it on the host
    ctx->phase_pending.clear();
    GDML_TRY(gdml_predict_virial_cells_dev(ctx, d_R, B, d_L, d_Li, d_Et, d_Ft, d_Wt));
    cell_update_kernel<<<(unsigned)B, 256, 0, st>>>(K, C, S, sl, cs, A, te, last);
    return (int)GDML_OK;
  }));
  DROP_HIP(hipMemcpy2DAsync(Sr, (size_t)n3a * 8, d_U, (size_t)n3 * 8, (size_t)n3a * 8, (size_t)B, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpy2DAsync(Cc, 72, d_U + n3a, (size_t)n3 * 8, 72, (size_t)B, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(V, d_V, (size_t)nu * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(R_end, d_R, (size_t)na * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(lat_end, d_L, (size_t)B * 72, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(F_end, d_Fe, (size_t)na * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(W_end, d_We, (size_t)B * 72, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(vol_end, d_ve, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(hipMemcpyAsync(E_end, d_E, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  DROP_HIP(d_fire.copy(h_fire, B, true, st));
  DROP_HIP(hipStreamSynchronize(st));
  // a frozen geometry repeats its last history values, its end positions and its end lattice up to the last evaluation made
  const TrajFrames frames[2] = {{R_rec, R_end, n3a}, {lat_rec, lat_end, 9}};
  fr.finish(status, first_bad_step, frames, 2);
  return drop(GDML_OK);
}

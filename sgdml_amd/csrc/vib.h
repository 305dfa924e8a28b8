// What gdml_vib_run (vib.hip) and gdml_ef_run (ef.hip) share, all of it defined in vib.hip: the spectrum of a slice of
// geometries (Hessian, projection, eigensolver, finish), the carving of its workspace (SpectrumWs, sym_eig_plan.h) and the
// argument checks both make; and the block sum their kernels use.
#pragma once
#include "sym_eig.h"
#include "traj.h"

// a slice's workspace carved: what spectrum_slice fills for the geometries of the slice
struct Spectrum {
  double *work, *H, *R, *F, *w, *info, *E, *mass;  // R: null where the positions belong to the run (gdml_ef_run)
  int64_t *sweeps, *n_rigid, *n_neg;
};

static inline Spectrum spectrum_carve(double* buf, const SpectrumWs& ws) {
  return {buf + ws.work, buf + ws.H, ws.with_R ? buf + ws.R : nullptr, buf + ws.F, buf + ws.w, buf + ws.info, buf + ws.E,
          buf + ws.mass, (int64_t*)(buf + ws.sweeps), (int64_t*)(buf + ws.n_rigid), (int64_t*)(buf + ws.n_neg)};
}

struct SpectrumIn {
  int N, project;
  double h_scale;
  const double *lat, *lat_inv;
};

// Queues the spectrum of the bc geometries d_R (bc, 3N) on the device: H', E', F' (gdml_predict_hessian_dev), the projection
// in place on H' (S.mass holds the masses), the eigen-launch of `plan` with its grid cut to bc (eigenvectors over D_s), the
// finish.  Three kernels behind the Hessian's own, counted here (the eigen-kernel by its launcher); no synchronisation.
int spectrum_slice(gdml_ctx* ctx, const SymEigPlan& plan, const Spectrum& S, const SpectrumIn& in, const double* d_R, int64_t bc);

// The argument checks of both entries, with the messages each has always given, in three pieces because each entry has always
// made them at three places among its own (a call with several bad arguments reports the one it always did):
//   projection  project in 0 .. 2, lattice and inverse both or neither, "project = 2 with a lattice"
//   atoms       the Hessian's atom limit
//   finite      the scan of the coordinates R (B, 3N), not null -- with t (B, 3N; may be null) the follow vector is scanned
//               entry by entry beside them
int spectrum_check_projection(gdml_ctx* ctx, const char* fn, int project, const double* lat, const double* lat_inv);
int spectrum_check_atoms(gdml_ctx* ctx, const char* fn, int N);
int spectrum_check_finite(gdml_ctx* ctx, const char* fn, int N, int64_t B, const double* R, const double* t);

// sum of one value per thread by the 256-slot tree, the same on every thread
__device__ __forceinline__ double vib_sum(double (*red)[256], int tid, double v) {
  red[0][tid] = v;
  __syncthreads();
  block_tree_sum<1>(red, tid);
  const double s = red[0][0];
  __syncthreads();
  return s;
}

// Host-side plan of the batched Jacobi eigensolver (sym_eig.hip) and of the spectrum of a slice of geometries built on it
// (spectrum_slice, vib.hip; called by gdml_vib_run and gdml_ef_run): storage route, LDS bytes, grid and work matrices of a
// launch, geometries per slice, and the layout of a slice's workspace.  Plain C++ with no HIP include and no gdml_ctx, so that
// the decision is a value one can print and test without a GPU (tests/sym_eig_plan_driver.cpp, tests/test_sym_eig_plan_cpu.py).
//
// STORAGE.  One workgroup of 256 threads per matrix.  Its LDS holds cs [npairs][2] doubles, pq [npairs][2] ints (padded to whole
// doubles) and red [8] doubles, then the working matrix A and the accumulated rotations V, N x NP doubles each, as far as they
// fit under 160 KiB: both for N <= 100, A alone for N <= 141, neither above that.  What does not fit lives in the workgroup's
// 2 x N x NP doubles of device memory (work_doubles covers every workgroup; nothing when V is in LDS).
// GRID.  4, 2 or 1 workgroups per compute unit by the LDS one takes, at most M.  cap_global is the one difference between the
// two callers: the full solver (gdml_sym_eig*, spectrum_slice) keeps the device-memory route at one workgroup per compute unit
// (its work matrices are 16 N^2 bytes per workgroup), the symmetry search (gdml_sym_eig_absv, gdml_perm_match) does not.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int VIB_MAX_ATOMS = 197;  // the Hessian's own limit
constexpr int SYM_EIG_MAX_N = 3 * VIB_MAX_ATOMS;
constexpr int64_t VIB_CHUNK_BYTES = 256ll << 20;
constexpr size_t SYM_EIG_LDS_MAX = 160 * 1024;

struct SymEigPlan {
  int NP;                  // row pitch of the working matrices (N + 1 when N is even: column accesses spread over the banks)
  int a_in_lds, v_in_lds;
  size_t lds;              // dynamic LDS bytes of a workgroup
  int64_t grid;            // workgroups (at most M)
  int64_t work_doubles;    // device memory behind the launch: grid x 2 x N x NP doubles, nothing when V is in LDS
};

static inline SymEigPlan sym_eig_plan(int num_cus, int64_t M, int N, bool cap_global) {
  SymEigPlan p;
  p.NP = (N % 2 == 0) ? N + 1 : N;
  const int ne = (N + 1) & ~1, npairs = ne / 2;
  const size_t fixed = (size_t)(2 * npairs) * 8 + (size_t)(2 * npairs + (npairs & 1) * 2) * 4 + 8 * 8;
  const size_t mat_b = (size_t)N * p.NP * 8;
  p.a_in_lds = fixed + mat_b <= SYM_EIG_LDS_MAX;
  p.v_in_lds = p.a_in_lds && fixed + 2 * mat_b <= SYM_EIG_LDS_MAX;
  p.lds = fixed + (p.a_in_lds ? mat_b : 0) + (p.v_in_lds ? mat_b : 0);
  p.grid = (int64_t)num_cus * (p.lds > 80 * 1024 ? 1 : p.lds > 40 * 1024 ? 2 : 4);
  if (p.grid > M) p.grid = M;
  if (cap_global && !p.a_in_lds && p.grid > num_cus) p.grid = num_cus;
  p.work_doubles = p.v_in_lds ? 0 : p.grid * 2 * (int64_t)N * p.NP;
  return p;
}

// The workspace of a slice of `len` geometries of N atoms, in doubles (every field is 8-byte words), in this order:
//   work matrices | H (D_s, then the eigenvectors) | [R] | F' | w | info (4 per geometry) | E' | mass (N) | sweeps | n_rigid | n_neg
// R is part of the slice for gdml_vib_run, which uploads a slice's geometries; for gdml_ef_run the positions belong to the run.
struct SpectrumWs {
  int64_t work, H, R, F, w, info, E, mass, sweeps, n_rigid, n_neg;  // offsets (R: that of F when with_R is 0)
  int with_R;
  int64_t per_geometry;  // doubles a geometry adds: everything but the work matrices and the masses
  int64_t total;
};

static inline SpectrumWs spectrum_ws(int64_t len, int N, int64_t work_doubles, bool with_R) {
  const int64_t n3 = 3 * (int64_t)N;
  SpectrumWs s;
  int64_t o = 0;
  const auto take = [&o](int64_t n) { const int64_t at = o; o += n; return at; };
  s.with_R = with_R;
  s.work = take(work_doubles);
  s.H = take(len * n3 * n3);
  s.R = take(with_R ? len * n3 : 0);
  s.F = take(len * n3);
  s.w = take(len * n3);
  s.info = take(len * 4);
  s.E = take(len);
  s.mass = take(N);
  s.sweeps = take(len);
  s.n_rigid = take(len);
  s.n_neg = take(len);
  s.total = o;
  s.per_geometry = len > 0 ? (o - work_doubles - N) / len : 0;
  return s;
}

// Geometries per chunk of gdml_vib_run and per slice of gdml_ef_run: Hessians, spectra and the eigensolver's work matrices
// under VIB_CHUNK_BYTES, whole slices of the Hessian's 64 when there are several; option (predict.vib_chunk) > 0 sets it.
// (a matrix beyond LDS brings its workgroup's two work matrices; beyond one workgroup per compute unit that over-counts)
static inline int64_t spectrum_slice_len(int num_cus, int64_t B, int n3, int64_t option) {
  const SymEigPlan p1 = sym_eig_plan(num_cus, 1, n3, true);
  const int64_t per = (spectrum_ws(1, n3 / 3, p1.work_doubles, true).per_geometry + p1.work_doubles) * 8;
  int64_t chunk = VIB_CHUNK_BYTES / per;
  if (chunk > 64) chunk = chunk / 64 * 64;
  if (option > 0) chunk = option;
  if (chunk < 1) chunk = 1;
  if (chunk > B) chunk = B;
  return chunk;
}

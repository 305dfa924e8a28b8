// Kernel-matrix assembly: the request every assembly kernel is asked with, and the two functions each kernel file exposes.
// The routing itself -- which kernel serves which request -- is the table in assemble.hip and nowhere else.
#pragma once
#include "common.h"

// What to assemble and where to write it.  Blocks (i, j) of row points [i_beg, i_end) and the selected column points.
struct AsmJob {
  double sig = 0.0;
  int use_E = 0;  // also write the energy-constraint ROW of every row point under the selected columns (train.py:235-248)
  // column selection: the dense point range [j0, j0 + n_j) written from output column 0, or n_j listed points (d_jlist)
  // with the output column of each of their 3N columns, -1 = not requested (d_colmap; h_colmap: its host copy or null)
  int64_t j0 = 0, n_j = 0;
  const int32_t *d_jlist = nullptr, *d_colmap = nullptr, *h_colmap = nullptr;
  int64_t i_beg = 0, i_end = 0;  // rows are stored relative to i_beg
  double* K = nullptr;
  int64_t ld = 0;
  // form: 0 = K, every block; 1 = A = -K + lam I, blocks j <= i only (needs the dense full range, asm_full_dense)
  int lower = 0;
  double lam = 0.0;
  // block-row-cyclic local layout of the distributed Cholesky (implies the lower form): row block b (nb rows) lives on rank
  // b % W as local row block b / W.  W = 0: plain.  W = 1 stores every row where the plain layout does; the distributed
  // solve asks with it on one rank, and assemble_wave then still runs its cyclic instantiation.
  int W = 0, rank = 0, nb = 0;
};

static inline bool asm_has_lists(const AsmJob& j) { return j.d_jlist || j.d_colmap; }
// rows land where the plain layout puts them: every kernel but assemble_wave / assemble_perm needs that
static inline bool asm_plain_rows(const AsmJob& j) { return j.W <= 1; }
// the dense full column range over all row points, forces only: the only request the lower form exists for
static inline bool asm_full_dense(const gdml_ctx* ctx, const AsmJob& j) {
  const int64_t M = ctx->ts.M;
  return !asm_has_lists(j) && !j.use_E && j.j0 == 0 && j.i_beg == 0 && j.n_j == M && j.i_end == M;
}
// The energy-constraint row / column entry of row point i is row e_row0 + i of the stored matrix: 3N M, or, with row-sharded
// storage (a rank holds the force rows of its points followed by THEIR energy rows), 3N (i_end - i_beg) - i_beg.
static inline int64_t asm_e_row0(int64_t M, int N, int64_t i_beg, int64_t i_end) {
  return (i_beg == 0 && i_end == M) ? M * 3 * (int64_t)N : (i_end - i_beg) * 3 * (int64_t)N - i_beg;
}
// Algorithmic bytes of one launch for ktime_end: every requested element written once (lower form: the n_i (n_i + 1) / 2
// blocks with j <= i).
static inline double asm_bytes(int N, bool lower, int64_t n_i, int64_t n_j) {
  const double blocks = lower ? 0.5 * (double)n_i * (double)(n_i + 1) : (double)n_i * (double)n_j;
  return 8.0 * blocks * 9.0 * N * N;
}

// Per kernel file: accepts() holds EVERY condition under which the kernel may take the job (shape, options and request);
// launch() assumes it held, that the job is not empty and that the dense tables are built (assemble_dispatch sees to both),
// and may still return GDML_ERR_UNSUPPORTED for what only its planning can tell (no LDS layout): the next kernel of the
// table is then tried.
bool assemble_strip_accepts(const gdml_ctx* ctx, const AsmJob& job);
int assemble_strip_launch(gdml_ctx* ctx, const AsmJob& job);
bool assemble_wave_accepts(const gdml_ctx* ctx, const AsmJob& job);
int assemble_wave_launch(gdml_ctx* ctx, const AsmJob& job);
bool assemble_pts_accepts(const gdml_ctx* ctx, const AsmJob& job);
int assemble_pts_launch(gdml_ctx* ctx, const AsmJob& job);
bool assemble_big1_accepts(const gdml_ctx* ctx, const AsmJob& job);
int assemble_big1_launch(gdml_ctx* ctx, const AsmJob& job);
bool assemble_perm2_accepts(const gdml_ctx* ctx, const AsmJob& job);
int assemble_perm2_launch(gdml_ctx* ctx, const AsmJob& job);
bool assemble_perm_accepts(const gdml_ctx* ctx, const AsmJob& job);
int assemble_perm_launch(gdml_ctx* ctx, const AsmJob& job);

int build_dense_tables(gdml_ctx* ctx);  // assemble_wave.hip: XF / GD of the resident training set, built once per upload
int assemble_dispatch(gdml_ctx* ctx, const AsmJob& job);
// energy-constraint rows of the block-row-cyclic layout (not part of the table: a separate step after it)
int assemble_erows_cyclic_launch(gdml_ctx* ctx, double sig, double lam, double* K, int64_t ld, int cyc_W, int cyc_rank,
                                 int cyc_nb);

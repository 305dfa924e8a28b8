// Internal definitions shared by the HIP translation units of libgdml_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/gdml_hip.h"

// Sanity bound on the molecule size, not a kernel limit: 32-bit index arithmetic over the N x N x 3 dense tables and the
// D = N (N - 1) / 2 descriptor rows holds far beyond it; memory (M N^2 32 bytes of dense tables) ends earlier.
#define GDML_MAX_ATOMS 4096

// periodic cell handed to the descriptor code by value (desc.hip, the single-launch prediction path of predict.hip)
struct Lattice {
  double lat[9];
  double inv[9];
  int use;
};

struct PhaseStat {
  double ms = 0.0;
  int64_t launches = 0;
};

// Per-kernel accumulators filled when profiling is enabled (gdml_profile): HIP events are
// recorded around every launch of the named kernel on the compute stream.
struct KernelStat {
  double ms = 0.0;       // sum of launch durations
  int64_t launches = 0;
  double work = 0.0;     // algorithmic work (flops or bytes) summed over launches
};
struct PendingTiming {
  std::string name;
  hipEvent_t e0, e1;
  double work;
};

// Device-resident training set (gdml_train_upload).
struct TrainSet {
  int64_t M = 0;
  int N = 0, D = 0, P = 0;
  double* x = nullptr;       // (M,D)    descriptors
  double* g = nullptr;       // (M,D,3)  compressed Jacobians
  int32_t* tp = nullptr;     // (P,D)    descriptor permutations
  int32_t* perm = nullptr;   // (P,N)    atom permutations  pi_p
  int32_t* pinv = nullptr;   // (P,N)    inverse atom permutations
  double* XF = nullptr;      // (M,N,N)   dense x[pair(b,m)] table, m-major (assemble_wave.hip)
  double* GD = nullptr;      // (M,N,N,3) dense G(b,m) table, m-major
  double* TS = nullptr;      // (M,pitch) packed per-point image [GD | XF | x | 0-pad] staged by assemble_strip.hip
  uint8_t* p2 = nullptr;     // plan of assemble_perm2.hip (internal atom numbering, byte permutations, V-phase tasks)
  double* p2_TP = nullptr;   // (M,N,N,4) packed per-point tables in that numbering
  int p2_o[4] = {0, 0, 0, 0}, p2_nF = 0, p2_nFb = 0, p2_ntasks = 0, p2_npairs = 0, p2_key = 0;
  std::vector<int32_t> h_tp, h_perm, h_pinv;
};

// Device-resident model for prediction (gdml_predict_upload_model).
struct Model {
  int64_t M = 0;
  int N = 0, D = 0, P = 0;
  double sig = 0;
  double* xp = nullptr;    // (M*P,D) permuted training descriptors (predict.py:426-431)
  double* jap = nullptr;   // (M*P,D) permuted J_m alpha_m          (predict.py:433-441)
  double* ja = nullptr;    // (M,D)   unpermuted J alpha (scratch for set_alphas)
  double* aE = nullptr;    // (M*P)   alphas_E repeated per perm (predict.py:443-447) or null
  int32_t* tp = nullptr;   // (P,D)
  bool has_aE = false;
};

// Cached work buffers of ctx_slot.  A buffer belongs to its requester from the ctx_slot call to the end of that library call:
// everything that touches it is ordered on the context's streams inside the call, nothing is carried over to the next call,
// and a request that has to grow the buffer waits for ctx->stream before the old one is freed.  Requesters may therefore
// share a slot exactly when none of them runs, or is called, while another's pointer is still in use:
//   SLOT_PREDICT_WS   predict_fused, the three paths of predict_device and hess_device are alternatives of one call each;
//                     none calls another (matvec_device -> predict_device holds SLOT_MATVEC_OUT / _VREF, not this one)
//   SLOT_PRECON_GEMV  precon_apply_device alone, laid out by precon_apply_plan (precon_plan.h) for the form that is resident
//   SLOT_PRECON_MF    build_f32_form reads its flag back and synchronises before it goes on, and applies no preconditioner;
//                     precon_apply_mf calls matvec_device, which requests other slots only
//   SLOT_GRAM_WS/ROWS every caller of gram_workspace (gdml_uncert_cross, cov_run for the four gdml_predict_cov* entries, gdml_loo,
//                     gdml_evidence_grad, gdml_select_points) carves them anew and calls none of the others while it holds them
//                     (gdml_predict_cov_few hands a batch beyond its limit to gdml_predict_cov BEFORE it carves anything; its
//                     inverted diagonal blocks are the fixed part of SLOT_GRAM_WS and live for one call); tall_trsm in between
//                     requests SLOT_PANEL_TRSM only.  gdml_factor_extend / gdml_factor_remove release both: they were sized for n
//   SLOT_VIB_WS       gdml_sym_eig, gdml_sym_eig_dev (sym_eig.hip) and gdml_vib_run (vib.hip: a chunk laid out by SpectrumWs,
//                     sym_eig_plan.h) carve it anew and call none of the others; the Hessian call inside spectrum_slice
//                     holds the scratch buffer and SLOT_PREDICT_WS only
//   SLOT_EF_WS        gdml_ef_run alone (ef.hip): a slice laid out by SpectrumWs without R, then its state, which lives there
//                     for the whole call, across the Hessian calls of every evaluation (which hold the scratch buffer and
//                     SLOT_PREDICT_WS only)
enum CtxSlot {
  SLOT_PREDICT_WS = 0,      // row-split partials of F_x and E (predict_device, predict_fused); workspace of hess_device
  SLOT_MATVEC_OUT = 1,      // forces and energies of this rank's query points (matvec_device)
  SLOT_LEV_SCORES = 2,      // replicated leverage scores (lev_scores_to_host: gdml_nystroem_lev_scores, gdml_nystroem_factor)
  SLOT_PRECON_GEMV = 3,     // row-split partials and m-vectors of one preconditioner application (precon_apply_device)
  SLOT_PREDICT_STATS = 4,   // row statistics of the table for predict_mfma_kernel (predict_device)
  SLOT_PANEL_SAVE = 5,      // deferred write-back of two 64 x 64 diagonal blocks (panel_factor_steps)
  SLOT_LU_UT = 6,           // transposed panel of U (lu_factor_device)
  SLOT_WIDE_WS = 7,         // pair scalars, row statistics, padded tables and queries (predict_wide_device)
  SLOT_PANEL_TRSM = 8,      // prepared diagonal blocks of a panel (launch_panel_trsm)
  SLOT_WIDE_PARTS = 9,      // k-split partials of the F_x contraction (predict_wide_device)
  SLOT_PRECON_MF = 10,      // vectors of the matrix-free preconditioner (precon_apply_mf); "fits on every rank" flag (build_f32_form)
  SLOT_F32_GRAM_ROWS = 11,  // widened row chunk of the rounded factor (build_f32_form)
  SLOT_MATVEC_VREF = 12,    // coefficients back in the reference order (matvec_device, sharded with energy constraints)
  SLOT_GRAM_WS = 13,        // queries / coefficients, partial Gram tiles, staged output (gram_workspace)
  SLOT_GRAM_ROWS = 14,      // the (3N x chunk, padded to 128 rows) x K_ld row buffer (gram_workspace)
  SLOT_VIB_WS = 15,         // matrices, spectra and the eigensolver's work matrices of a chunk (gdml_sym_eig*, gdml_vib_run)
  SLOT_EF_WS = 16,          // state, end-of-run outputs, histories and a slice's matrices of gdml_ef_run
  SLOT_COUNT
};

struct TileSchedCache;  // balanced tile lists of the lower trailing updates and their device tables (chol.hip)

struct gdml_ctx {
  int device = 0;
  int num_cus = 256;  // compute units of the device (grid sizing)
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;
  hipStream_t kt_stream = nullptr;                       // stream the per-kernel timers record on (default: stream)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_la[6] = {};  // hand-offs between the two streams (look-ahead, overlapped panel solves)
  std::string err;
  std::map<std::string, double> opts;  // tuning / ablation options (gdml_set_option); absent key = built-in default
  int64_t held = 0;
  std::map<void*, int64_t> allocs;
  std::map<std::string, PhaseStat> phases;
  std::string phase_pending;         // phase whose end event has been recorded but not read yet
  int64_t phase_pending_launches = 0;
  double* h_pin = nullptr;           // pinned host staging for small transfers (single-geometry latency path)
  int64_t h_pin_bytes = 0;
  // single-launch prediction of small host batches (predict_fused_kernel): host-mapped result block the kernel writes
  // directly ([0] = completion sequence number, [8 ...] = E, F), its device alias, the launch counter of the last-block-done
  // reduction and the sequence number of the last launch
  double* h_map = nullptr;
  double* h_map_dev = nullptr;
  unsigned* d_fused_counter = nullptr;
  unsigned long long fused_seq = 0;
  int64_t launch_counter = 0;
  bool profiling = false;
  std::map<std::string, KernelStat> kstats;
  std::vector<PendingTiming> pending;
  std::vector<hipEvent_t> event_pool;

  TrainSet ts;
  Model model;

  // kernel matrix / Cholesky factor
  double* K = nullptr;
  int64_t K_rows = 0, K_cols = 0, K_extra = 0, K_ld = 0, K_bytes = 0;
  bool K_factored = false;
  bool K_destroyed = false; // a failed Cholesky or an LU consumed the buffer: assemble again before factoring
  bool K_is_A = false;      // the buffer already holds A = -K + lam I (lower blocks; gdml_assemble_A): factor skips the sign flip
  bool K_rhs_row = false;   // row K_rows of the buffer carries a right-hand side (gdml_chol_set_rhs)
  double* d_rhs = nullptr;  // device copy of that right-hand side (iterative refinement)
  double K_lam = 0, K_sig = 0;
  bool uncert_ready = false; // the factor in K is the one gdml_uncert_prepare built for the resident training set (uncert.hip)
  int K_use_E = 0;

  // Nystroem preconditioner L^-1 K_mn (m x n)
  double* precon = nullptr;
  int64_t precon_m = 0, precon_n = 0;
  // form of the resident preconditioner (option pcg.precon_form): 0 = the stored n x m factor X = K_nm Z is streamed twice
  // per application; 1 = matrix-free, P v = (K_nm Z Z^T K_mn v - v)/lam through two kernel mat-vecs and the m x m matrix
  // Z = L_mm^-T L^-T (nystroem.hip).  precon_stage: triangular solves applied to X so far (1: only L_mm^-T -- the matrix-free
  // form does not need the second one until somebody asks for leverage scores).
  int precon_form = 0, precon_stage = 2, precon_use_E = 0;
  double precon_sig = 0;
  double* precon_Z = nullptr;     // m x K_ld, upper triangular
  int64_t precon_Z_bytes = 0;
  int64_t* precon_idx = nullptr;  // device copy of the inducing column indices (m)
  int64_t precon_idx_bytes = 0;
  // form 3: the factor rounded to fp32 (n_loc x K_ld floats) + the m x m correction T0 that makes
  // (X32 T0 X32^T - I)/lam the exact Woodbury inverse on range(X32) (nystroem.hip)
  float* precon_X32 = nullptr;
  int64_t precon_X32_bytes = 0;
  bool precon_X32_inplace = false;        // X32 overlays the fp64 factor in the matrix buffer (row pitch 2 K_ld floats): not ours to free
  int64_t precon_X32_ld = 0;              // row pitch of X32 in floats
  std::vector<double> precon_lev_cache;   // leverage scores taken before the in-place rounding
  double* precon_T0 = nullptr;
  int64_t precon_T0_bytes = 0;

  // scratch
  double* scratch = nullptr;
  int64_t scratch_bytes = 0;
  double* slot[SLOT_COUNT] = {};  // cached work buffers (ctx_slot, CtxSlot)
  int64_t slot_bytes[SLOT_COUNT] = {};
  int* d_info = nullptr;
  TileSchedCache* tile_sched = nullptr;

  // comm
  void* comm = nullptr;  // ncclComm_t
  void* comm2 = nullptr; // second communicator over the same ranks (ncclCommSplit): latency-critical small broadcasts of the
                         // distributed Cholesky, so that they do not queue behind the panel all-gather on `comm`
  int rank = 0, world = 1;
  // gdml_comm_suspend: the communicator parked here while the context acts as a single GPU (redundant solves)
  struct {
    bool on = false;
    void *comm = nullptr, *comm2 = nullptr;
    int rank = 0, world = 1;
    bool virtual_rank = false;
    gdml_host_allreduce ar = nullptr;
    gdml_host_allgather ag = nullptr;
  } parked;
  bool virtual_rank = false;   // shard arithmetic only, collectives skipped (tests)
  gdml_host_allreduce host_allreduce = nullptr;  // host-staged collectives (gdml_comm_init_host)
  bool comm_aborted = false;  // comm_abort() ran: every later collective fails instead of acting like a single rank
  gdml_host_allgather host_allgather = nullptr;
  void* host_coll_user = nullptr;
  double* h_coll = nullptr;    // pinned staging buffer of the host-staged collectives
  int64_t h_coll_bytes = 0;
  int64_t coll_calls = 0;      // collectives issued (any backend) since gdml_comm_init*
  double coll_bytes = 0.0;     // payload bytes this rank handed to them
  bool K_sharded = false;      // resident K holds only this rank's rows (Nystroem path)
  int64_t K_rows_global = 0;
};

int gdml_fail(gdml_ctx* ctx, int code, const char* fmt, ...);
// option lookup (ctx.hip): value of `key`, or dflt when it was never set
double ctx_opt(const gdml_ctx* ctx, const char* key, double dflt);
static inline int ctx_opt_i(const gdml_ctx* ctx, const char* key, int dflt) { return (int)ctx_opt(ctx, key, (double)dflt); }

#define HIP_CHECK(ctx, call)                                                              \
  do {                                                                                    \
    hipError_t e__ = (call);                                                              \
    if (e__ != hipSuccess)                                                                \
      return gdml_fail(ctx, e__ == hipErrorOutOfMemory ? GDML_ERR_OOM : GDML_ERR_HIP,     \
                       "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__,  \
                       __LINE__);                                                         \
  } while (0)

#define GDML_TRY(expr)          \
  do {                          \
    int rc__ = (expr);          \
    if (rc__ != GDML_OK) return rc__; \
  } while (0)

// The same two for a function that owns buffers until it commits: they leave through a local callable `drop(rc)`, which
// frees what the call allocated and returns rc (gdml_select_points, gdml_factor_extend, gdml_factor_remove).
#define DROP_TRY(expr)                      \
  do {                                      \
    const int rc_e = (expr);                \
    if (rc_e != GDML_OK) return drop(rc_e); \
  } while (0)
#define DROP_HIP(call)                                                                                              \
  do {                                                                                                              \
    const hipError_t e_e = (call);                                                                                  \
    if (e_e != hipSuccess)                                                                                          \
      return drop(gdml_fail(ctx, e_e == hipErrorOutOfMemory ? GDML_ERR_OOM : GDML_ERR_HIP, "%s failed: %s (%s:%d)", \
                            #call, hipGetErrorString(e_e), __FILE__, __LINE__));                                    \
  } while (0)

// context-tracked allocation helpers (ctx.hip)
int ctx_alloc(gdml_ctx* ctx, void** p, int64_t bytes);
int ctx_free(gdml_ctx* ctx, void* p);
int ctx_scratch(gdml_ctx* ctx, int64_t bytes, double** out);
void phase_begin(gdml_ctx* ctx);
// kernel timing (no-ops unless ctx->profiling)
int phase_resolve(gdml_ctx* ctx);  // reads a pending phase timer (waits for its end event)
void precon_release_f32(gdml_ctx* ctx);  // nystroem.hip
void precon_release_aux(gdml_ctx* ctx);
// |eigenvectors| of M symmetric N x N matrices on the device, columns by decreasing eigenvalue: d_v [a][k], d_vT [k][a] (sym_eig.hip)
int sym_eig_absv_dev(gdml_ctx* ctx, const double* d_adj, double* d_v, double* d_vT, int64_t M, int N);
int ktime_begin(gdml_ctx* ctx);  // returns slot or -1
void ktime_end(gdml_ctx* ctx, int slot, const char* name, double work);
int ktime_collect(gdml_ctx* ctx);
int phase_end(gdml_ctx* ctx, const char* name);

static inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline int64_t round16(int64_t v) { return (v + 15) / 16 * 16; }  // pitches: rows start on 128-byte boundaries

// ---- device helpers -----------------------------------------------------------------
// index of the descriptor entry for the unordered atom pair {a,b}, a != b
__device__ __forceinline__ int pair_idx(int a, int b) {
  int hi = a > b ? a : b;
  int lo = a > b ? b : a;
  return (hi * (hi - 1)) / 2 + lo;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// load(0) + ... + load(n - 1), added in index order; loaded eight at a time, the index clamped to n - 1, so that a batch is
// eight independent loads behind one wait instead of a chain of load + wait per value
template <typename Int, typename Load>
__device__ __forceinline__ double sum_in_order8(Int n, Load load) {
  double s = 0.0;
  for (Int i0 = 0; i0 < n; i0 += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = load(i0 + u < n ? i0 + u : n - 1);
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (i0 + u < n) s += v[u];
  }
  return s;
}

// internal cross-TU entry points
int desc_device(gdml_ctx* ctx, const double* d_R, int64_t M, int N, const double* lat,
                const double* lat_inv, double* d_x, double* d_g);
int desc_cells_device(gdml_ctx* ctx, const double* d_R, int64_t M, int N, const double* d_lats, const double* d_invs,
                      double* d_x, double* d_g);  // a lattice per geometry, (M,3,3) in device memory
int predict_device(gdml_ctx* ctx, const double* d_xq, const double* d_gq, int64_t B, double* d_E,
                   double* d_F);
int hess_device(gdml_ctx* ctx, const double* d_xq, const double* d_gq, int64_t B, double* d_E, double* d_F,
                double* d_H);  // predict_hess.hip
int predict_wide_device(gdml_ctx* ctx, const double* d_xq, int64_t B, double* part_F, double* part_E);
int set_alphas_device(gdml_ctx* ctx, const double* d_alphas_F, const double* d_alphas_E);
int matvec_device(gdml_ctx* ctx, double lam, int use_E_cstr, const double* d_v, int64_t n,
                  double* d_out);
int chol_factor_device(gdml_ctx* ctx, double* A, int64_t n, int64_t ld, int* info, int64_t n_rows = 0);
int lu_factor_device(gdml_ctx* ctx, double* A, int64_t n, int64_t ld, int64_t* d_piv, int* info_out);
int chol_solve_device(gdml_ctx* ctx, const double* L, int64_t n, int64_t ld, double* d_b,
                      double* d_z, double* d_x);
int operator_model_from_trainset(gdml_ctx* ctx, double sig);
int launch_gemm_nt_sub(gdml_ctx* ctx, hipStream_t st, const double* A, int64_t lda, const double* B,
                       int64_t ldb, double* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int lower);
int launch_gemm_nt_neg(gdml_ctx* ctx, hipStream_t st, const double* A, int64_t lda, const double* B, int64_t ldb,
                       double* C, int64_t ldc, int64_t M, int64_t N, int64_t K);  // C = -A B^T (C is not read)
// lower structure of a block-row-cyclic local matrix (see GemmArgs in chol.hip)
struct CyclicLower {
  int W = 0, rank = 0;
  int64_t lb0 = 0, nb = 0, col0 = 0, block_rows = 0;
};
int launch_gemm_nt_sub_cyclic(gdml_ctx* ctx, hipStream_t st, const double* A, int64_t lda, const double* B, int64_t ldb,
                              double* C, int64_t ldc, int64_t M, int64_t N, int64_t K, const CyclicLower& cyc);
int launch_trsm64(gdml_ctx* ctx, hipStream_t st, const double* Ld, double* X, int64_t ld, int w,
                  int64_t m, int64_t ldl = 0);
int launch_panel_trsm(gdml_ctx* ctx, hipStream_t st, const double* L, double* X, int64_t ld, int nb, int64_t m,
                      int64_t ldl = 0);
int panel_factor_steps(gdml_ctx* ctx, hipStream_t st, double* A, int64_t n, int64_t ld, int64_t k0, int64_t nb);
int chol_bwd_device(gdml_ctx* ctx, const double* L, int64_t n, int64_t ld, double* d_z, double* d_x);
// X[:, 0:m] <- X L^-T for the n rows of X (chol_solve.hip).  look: 1 left-looking, 0 right-looking, -1 = option nys.trsm_left
int tall_trsm(gdml_ctx* ctx, const double* L, double* X, int64_t n, int64_t m, int64_t ld, int look = -1);
void tile_sched_cache_free(gdml_ctx* ctx);
int ctx_slot(gdml_ctx* ctx, int slot, int64_t bytes, double** out);
int ctx_slot_release(gdml_ctx* ctx, int slot);
// ---- the resident Cholesky factor and what is computed from it ---------------------------------------------------------------
// the k-split plan of a block Gram over n columns (block_gram.hip); also the shape a resident factor of n rows must have
struct GramSplit {
  int n3, nblk, npairs, S;  // rows of an item, its 64-row blocks and lower block pairs, k splits
  int64_t n, ld, L;         // columns, pitch (n rounded up to 16), split length
};
GramSplit gram_split(int64_t n, int n3);
// The contract of the entries that work on the factor in ctx->K, checked in this order: a training set is
// resident (GDML_ERR_STATE), the factor carries no energy-constraint rows (GDML_ERR_UNSUPPORTED), a factor is resident --
// need_prepared: the one gdml_uncert_prepare built -- (GDML_ERR_STATE), and it is the square, unsharded 3N M x 3N M factor of
// the resident training set at pitch round16(3N M) (GDML_ERR_STATE).  Fills g_out from gram_split.  Nothing is allocated and
// nothing is launched.  The rank test of a caller that has one stays in front of it.  (resident.hip)
int resident_factor_check(gdml_ctx* ctx, const char* who, bool need_prepared, GramSplit* g_out);
// Rows 3N j0 .. 3N (j0 + bc) - 1 of L^-T into `rows` (pitch g.ld): zeroed and seeded with E^T from column c0 = the first row
// index rounded down to the 512-column panel grid of tall_trsm, then solved on the trailing sub-problem from c0, right-looking,
// on whole 128-row tiles (columns left of c0 are neither written nor read).  The two steps are timed as t_seed / t_solve;
// with `keep` the true rows (not the pad rows) are also copied to their place in that n x g.ld matrix, inside t_solve.
int factor_inverse_rows(gdml_ctx* ctx, const GramSplit& g, double* rows, int64_t j0, int64_t bc, const char* t_seed,
                        const char* t_solve, double* keep = nullptr);
// log det A = 2 sum log L_ii: a strided gather into d_diag (g.n doubles) and a host sum in index order
int factor_logdet(gdml_ctx* ctx, const GramSplit& g, double* d_diag, double* logdet_out);
// The commit of gdml_factor_extend / gdml_factor_remove: Kn (n1 rows, pitch ld1) replaces the resident factor and x1, g1 (M1
// points) the descriptor tables; the tables derived from the old training set are freed (an assembly builds them again).
// The stream is idle and every pointer is tracked: nothing here fails half way.
void factor_commit(gdml_ctx* ctx, double* Kn, int64_t Kn_bytes, int64_t n1, int64_t ld1, double* x1, double* g1, int64_t M1);

// ---- block Gram of tall row blocks (block_gram.hip), the chunking of such blocks and the posterior-covariance chunk (uncert.hip)
// The solve runs on whole 128-row tiles (zero rows behind the last item): an interior tile of the trailing update and an
// edge tile round differently (chol.hip: acc = -C first vs C - acc last), and which of the two an item's rows meet must not
// depend on how the items were cut into chunks.
static inline int64_t pad_rows128(int64_t rows) { return (rows + 127) / 128 * 128; }
// chunk length (option chunk_opt, default 64, less when free memory is short), row buffer and workspace of ws_fixed +
// chunk * ws_per_item doubles
int gram_workspace(gdml_ctx* ctx, const GramSplit& g, const char* chunk_opt, int64_t items, int64_t ws_per_item, int64_t ws_fixed,
                   int64_t* chunk, double** rows, double** ws);
// partial tiles of Z_i Z_i^T for `items` row blocks; item i is zero left of column first0 + i first_stride.  One launch, not timed.
// pitch: row pitch of Z when it is not g.ld (0 = g.ld)
void block_gram_launch(gdml_ctx* ctx, const GramSplit& g, const double* Z, double* part, int64_t items, bool diag, int64_t first0,
                       int64_t first_stride, int64_t pitch = 0);
// sgn * (cross-kernel rows) of bc device-resident queries against M column points, and sgn * k_qq unless kqq is null
// (uncert.hip; extend.hip, select.hip)
int cross_rows_launch(gdml_ctx* ctx, const double* xt, const double* gt, int64_t M, const double* xq, const double* gq, int bc,
                      double* rows, int64_t ld, double* kqq, double sgn, double sig, const char* tname);
// out = sym(-k_qq) - sum_s partial_s of `items` row blocks whose partial tiles block_gram_launch wrote (uncert.hip; select.hip)
void cov_reduce_launch(gdml_ctx* ctx, const GramSplit& g, const double* part, const double* nkqq, double* out, int64_t items,
                       int full);
// Sig_q = (-k_qq) - Z_q Z_q^T, Z_q = (-Kx_q) L^-T for a chunk of queries (uncert.hip; uncert_few.hip, select.hip).
// CovChunk: the per-chunk work buffers, R | xq | gq | nkqq | out | part, cov_chunk_doubles per query (part only with gram).
// cov_chunk_carve lays them out from ws for chunks of at most bc queries and returns the first double behind them.
struct CovChunk {
  double *R, *xq, *gq, *nkqq, *out, *part;
};
int64_t cov_chunk_doubles(const GramSplit& g, int64_t D, bool gram);
double* cov_chunk_carve(CovChunk* c, double* ws, const GramSplit& g, int64_t D, int64_t bc, bool gram);
// What tells the users of the chunk step apart: the timer names, and the solve.  solve == nullptr: tall_trsm, right-looking, on
// rows padded to 128, timed as t_solve.  Otherwise solve(ctx, g, rows, rows_pad, work, fixed) on rows padded to row_pad, which
// times itself; `fixed` is its part of the workspace (ws_fixed doubles in front of the chunk buffers).
struct CovPath {
  const char *t_cross, *t_solve, *t_gram, *phase;
  int row_pad;
  int (*solve)(gdml_ctx* ctx, const GramSplit& g, double* rows, int64_t rows_pad, double work, double* fixed);
};
// One chunk: [upload R] -> descriptors -> cross_rows_launch -> zero the pad rows -> solve -> block_gram_launch ->
// cov_reduce_launch into d_out ((bc,3N,3N) with full, else (bc,3N), on the device).  R: bc geometries, on the host unless R_on_device.
int cov_chunk_step(gdml_ctx* ctx, const GramSplit& g, const CovPath& path, const CovChunk& c, double* rows, double* fixed,
                   const double* R, bool R_on_device, int bc, const double* lat, const double* lat_inv, int full, double* d_out);
// the argument and state checks of the four gdml_predict_cov* entries, and their chunk loop (carves the Gram slots)
int cov_check(gdml_ctx* ctx, const char* who, const double* R, int64_t B, const double* lat, const double* lat_inv,
              const double* cov_out, GramSplit* g_out);
int cov_run(gdml_ctx* ctx, const GramSplit& g, const CovPath& path, const double* R, bool on_device, int64_t B, const double* lat,
            const double* lat_inv, int full, double* cov_out, int64_t ws_fixed = 0);
void shard_points(const gdml_ctx* ctx, int64_t M, int64_t* p0, int64_t* p1, int64_t* pts_per);
// Layout of the replicated device vectors of the sharded solvers (Nystroem factor rows, PCG vectors, mat-vec in / out).
//   no communicator (world <= 1): the reference order, n entries, no padding;
//   sharded, forces only: the reference order padded to world * chunk, chunk = 3N per (per = points per rank): a rank's
//     rows [row0, row0 + n_loc) are one contiguous run and one all-gather of `chunk` entries replicates a result;
//   sharded WITH energy constraints (round 6; train.py:235-300 appends the M energy entries behind the 3N M force entries):
//     rank-major -- rank r's chunk of (3N + 1) per entries = [force entries of its points | their energy entries | padding] --
//     so that a rank's n_loc local rows are STILL one contiguous run and everything between the boundaries (factor rows,
//     GEMVs, all-gathers, CG vector updates over n_pad entries with zero padding) runs unchanged.  The order exists only
//     inside the library: vectors are permuted where they enter / leave (vec_upload / vec_download, pos()).
struct VecLayout {
  int64_t n = 0, n_ff = 0, M = 0, N3 = 0, per = 0;
  int64_t chunk = 0, n_pad = 0, row0 = 0, n_loc = 0;
  int two_seg = 0;
  __host__ __device__ int64_t pos(int64_t g) const {  // reference index -> position in the device vector
    if (!two_seg) return g;
    if (g < n_ff) {
      const int64_t pt = g / N3, r = pt / per;
      return r * chunk + (pt - r * per) * N3 + (g - pt * N3);
    }
    const int64_t e = g - n_ff, r = e / per;
    const int64_t cnt = (M - r * per < per) ? M - r * per : per;
    return r * chunk + cnt * N3 + (e - r * per);
  }
};
VecLayout vec_layout(const gdml_ctx* ctx, int use_E_cstr);
// ---- Nystroem preconditioner and PCG: gram_tn.hip, nystroem.hip, precon_apply.hip, cg.hip
// C (m x m, lower tiles) = X^T X over the n rows of X, cut along the rows where that pays (gram_tn.hip); the one-pass kernel
// alone, launched and not checked
int gram_tn(gdml_ctx* ctx, const double* X, int64_t ldx, int64_t n, int64_t m, double* Cout, int64_t ldc);
void launch_gram_one_pass(gdml_ctx* ctx, const double* X, int64_t ldx, int64_t rows, int64_t m, double* C, int64_t ldc);
// row-shard geometry of the resident Nystroem matrix (nystroem.hip)
typedef VecLayout ShardGeo;
ShardGeo shard_geo(const gdml_ctx* ctx);
// d_out = P d_v on replicated (padded) device vectors, in the resident form (precon_apply.hip)
int precon_apply_device(gdml_ctx* ctx, double lam, const double* d_v, double* d_out);
// y += a x over n entries (cg.hip), launched and not checked
void launch_vec_axpy(gdml_ctx* ctx, double* y, const double* x, double a, int64_t n);
// host vector (reference order, L.n entries) -> zero-padded device vector of L.n_pad entries, and back (synchronous)
int vec_upload(gdml_ctx* ctx, const VecLayout& L, const double* host_ref, double* dev);
int vec_download(gdml_ctx* ctx, const VecLayout& L, const double* dev, double* host_ref, hipStream_t st = nullptr);
int comm_allgather_inplace(gdml_ctx* ctx, double* buf, int64_t chunk);
int comm_allreduce_sum(gdml_ctx* ctx, double* buf, int64_t count);
int comm_allgather_inplace_on(gdml_ctx* ctx, double* buf, int64_t chunk, hipStream_t st);
int comm_broadcast_on(gdml_ctx* ctx, double* buf, int64_t count, int root, hipStream_t st, bool second_comm = false);
void comm_destroy(gdml_ctx* ctx);
int comm_ensure_second(gdml_ctx* ctx);
// A rank that fails locally between collectives (a launch error in a panel loop) must not leave its peers blocked in
// the collective it will never join: RCCL communicators are aborted (ncclCommAbort: the peers' pending and later
// operations end with an error), and this context refuses further collectives.
void comm_abort(gdml_ctx* ctx);
static inline bool comm_active(const gdml_ctx* ctx) { return (ctx->comm || ctx->host_allreduce) && !ctx->virtual_rank; }

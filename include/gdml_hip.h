/*
 * gdml_hip.h -- C ABI of libgdml_hip.so: the MI355X (gfx950) implementation of sGDML's
 * kernel linear-algebra hot path.
 *
 * This is the drop-in boundary.  Every entry point replaces one
 * NumPy / SciPy / PyTorch call site of the reference (cited as file:line relative to the
 * reference repository root); the Python classes in sgdml_amd/ bind them with ctypes and
 * keep the reference's public API (GDMLTrain / GDMLPredict / Analytic / Iterative).
 *
 * Conventions
 *   - plain C: opaque context pointer, host pointers to float64 / int64 row-major (C-order)
 *     arrays owned by the caller unless a parameter is documented as a DEVICE pointer;
 *   - every function returns 0 on success or a negative gdml_status; it never throws and
 *     never calls exit(); gdml_last_error() returns a human-readable description;
 *   - one context per GPU; a context is not thread-safe, different contexts are independent;
 *   - all arithmetic is IEEE float64 (the reference computes in float64 everywhere:
 *     sgdml/torchtools.py:49, sgdml/train.py:1484, sgdml/predict.py:80);
 *   - N = atoms, D = N(N-1)/2 descriptor entries in np.tril_indices(N,-1) order
 *     (sgdml/utils/desc.py:264), M = training points, P = permutations, dim_i = 3N.
 */
#ifndef GDML_HIP_H
#define GDML_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gdml_ctx gdml_ctx;

typedef enum {
  GDML_OK = 0,
  GDML_ERR_INVALID = -1,     /* bad argument (maps to ValueError / AssertionError)        */
  GDML_ERR_HIP = -2,         /* HIP runtime error                                          */
  GDML_ERR_OOM = -3,         /* device allocation failed (reference: OOM re-batching,
                                sgdml/torchtools.py:349-387; here the host decides)        */
  GDML_ERR_STATE = -4,       /* call order violated (e.g. solve before assemble)          */
  GDML_ERR_NOT_PD = -5,      /* Cholesky met a non-positive pivot (LinAlgError analogue,
                                sgdml/solvers/analytic.py:101)                            */
  GDML_ERR_UNSUPPORTED = -6, /* size beyond what this build's kernels support             */
  GDML_ERR_COMM = -7         /* RCCL failure                                               */
} gdml_status;

/* ---- library / context --------------------------------------------------------------- */

/* ABI version of this header (bumped on any signature change). */
int gdml_abi_version(void);

/* Number of visible HIP devices (reference: torch.cuda.device_count(), train.py:1464). */
int gdml_device_count(int* n_out);

/* PCI bus id ("0000:c1:00.0") of visible device `device` into out[len >= 16]: the physical identity of a GPU, so that
 * ranks whose launcher gave each of them a private one-device view can still tell whether they share a GPU (RCCL
 * refuses duplicate devices).  No reference counterpart (the reference is single-process). */
int gdml_device_pci_bus_id(int device, char* out, int len);

/* Create / destroy the per-GPU context: owns one compute stream, one copy stream, all
 * device buffers and (after gdml_comm_init) the RCCL communicator. */
int gdml_ctx_create(int device, gdml_ctx** ctx_out);
int gdml_ctx_destroy(gdml_ctx* ctx);

/* Last error text of a context (ctx may be NULL: text of the last failed gdml_ctx_create). */
const char* gdml_last_error(const gdml_ctx* ctx);

/* Block until all work queued on the context's streams has finished. */
int gdml_sync(gdml_ctx* ctx);

/* Device memory currently held by the context, and free/total HBM of its device (bytes). */
int gdml_mem_info(gdml_ctx* ctx, int64_t* held, int64_t* free_b, int64_t* total_b);

/* Process-level device arena: reserve ONE block of `bytes` on the context's device and keep it until the process ends
 * (or until gdml_mem_reserve(ctx, 0, ...), which fails with GDML_ERR_STATE while any buffer is carved from it).  The large
 * buffers (>= 1 GiB) of every context on that device -- the kernel matrix, the Nystroem matrix, the fp32 copy of the
 * preconditioner factor -- are carved from it first-fit instead of hipMalloc / hipFree, which cost seconds per call beyond
 * ~128 GB on this driver; the block survives gdml_ctx_destroy.  A request that fits no gap goes to hipMalloc.  gdml_mem_info
 * counts the idle part of the arena as free.  reserved_out: bytes now held.
 * (The reference sizes its work to host RAM, sgdml/train.py:949-964; there is nothing to mirror here.) */
int gdml_mem_reserve(gdml_ctx* ctx, int64_t bytes, int64_t* reserved_out);

/* Elapsed milliseconds (HIP events on the compute stream) of the most recent call of the
 * named phase: "desc", "assemble", "factor", "solve", "predict", "matvec", "precon", "uncert", "loo", "evidence".
 * Also returns how many kernel launches the phase issued. */
int gdml_phase_ms(gdml_ctx* ctx, const char* phase, double* ms_out, int64_t* launches_out);

/* Per-kernel timing for roofline reports: after gdml_profile(ctx, 1) every launch of the hot
 * kernels is bracketed by HIP events on the compute stream; gdml_kernel_stat returns the summed
 * launch duration, the launch count and the summed ALGORITHMIC work (flops for "gemm_nt_sub",
 * bytes for "assemble" and "predict") since profiling was enabled.  Off by default.
 * "gemm_nt_sub_diag" covers every trailing-update launch that carries a diagonal block, the composed launches of
 * chol.deep included.  "gemm_nt_sub_deep" is a COUNT only: launches that held far tiles and those tiles' flops, with
 * ms = 0 (their time is part of "gemm_nt_sub_diag"): do not form a rate from it. */
int gdml_profile(gdml_ctx* ctx, int enable);
int gdml_kernel_stat(gdml_ctx* ctx, const char* kernel, double* ms_out, int64_t* launches_out,
                     double* work_out);

/* Tuning / ablation options of a context (all have built-in defaults; nothing here changes results beyond
 * rounding).  Read at the point of use, so a value set between two calls applies to the next call.  The
 * library reads no environment variables except GDML_OPTIONS="key=value,..." (applied at gdml_ctx_create).
 *   asm.wave (1)          register-resident assembly kernel for P = 1, N <= 21 (0: the general kernel); asm.j_chunk its
 *                         column points per workgroup
 *   asm.lower (1)         analytic path: assemble only blocks on/below the diagonal, as -K + lam I
 *   asm.strip (1)         64-column-strip assembly kernel (full-line stores) for P = 1, 11 <= N <= 21, all columns
 *   asm.i_chunk (32)      row points walked by one wavefront of the strip kernel
 *   asm.pts (1; 2 = also for P = 1) small molecules (8 <= N <= 24) with a permutation group: whole-point strips, producer / consumer
 *                         wavefronts (csrc/assemble_pts.hip); asm.pts_nv (0 = automatic) producer wavefronts, asm.pts_nt (1) non-temporal stores of K, asm.pts_xcd (1) adjacent strips on one XCD, asm.pts_i_chunk (64)
 *                         row points per workgroup, asm.pts_debug (0) timing-only ablation mask (results are wrong when set)
 *   general assembly kernel (any permutation group, any N: column-atom strips, csrc/assemble_perm.hip):
 *   asm.perm_level (-1 = automatic: 0 nothing, 1 row-point image, 2 + G_j strip, 3 + x_j tables resident in LDS),
 *   asm.perm_debug (0)    timing-only ablation mask of that kernel (results are wrong when set)
 *   asm.perm_w (0 = automatic: 4 wavefronts per workgroup for N <= 24, else 8), asm.perm_lds_kb (80: per workgroup of 4),
 *   asm.perm_nimg (0 = automatic), asm.perm_pg (0 = automatic), asm.perm_na (0 = automatic), asm.perm_fast_store (1),
 *   asm.perm_i_chunk (16) its shape: image buffers, permutations per group, row atoms per wavefront, transposed
 *                         full-line stores, row points per workgroup
 *   asm.perm_compact (1)  index-list columns: strips of the REQUESTED column atoms instead of all atoms of every point touched
 *   asm.perm_lds_rows (1) permutation entries from the LDS copy for 64 < N <= 128 (always beyond 128 atoms); 0 = two lane-held rows (A/B)
 *   asm.big1 (1)          no permutation group and 22 <= N <= 256, dense column range: the direct P = 1 kernel (assemble_big1.hip,
 *                         round 6) instead of the general permutation kernel; 0 = the general kernel (A/B)
 *   asm.perm2 (1)         molecules with a permutation group of at least asm.perm2_min_p (6) elements, asm.perm2_min_n (36) <= N <= 42
 *                         (groups below 16 elements: from 4 atoms more), dense column ranges -- where it beats the general kernel
 *                         (1.8x at N = 42, P = 27): outer products on
 *                         the fp64 MFMA pipe, contributions of atom pairs no permutation moves summed once per block
 *                         (csrc/assemble_perm2.hip); asm.perm2_split (1; 0 = every pair per permutation), asm.perm2_post (1: single and diagonal
 *                         terms that involve an atom no permutation moves summed over the permutations once per block; 0 = per permutation), asm.perm2_ed (1: diagonal terms of
 *                         moved atoms summed per (row atom, column atom) pair by idle lanes; needs asm.perm2_post), asm.perm2_es (1: single terms of
 *                         moved x moved blocks summed over the permutations once per block by four lanes per block; needs asm.perm2_post), asm.perm2_direct (1: finished rows stored straight
 *                         from the registers, 24 bytes per lane and row; 0 = through LDS in four passes of full-row stores), asm.perm2_chunk (12) pair
 *                         entries per lane and task, asm.perm2_i_chunk (16) row points per workgroup, asm.perm2_debug (0)
 *                         timing-only ablation mask (results are wrong when set)
 *   predict.wide_pad (1)  the same contractions on tables / queries padded to whole tiles (no edge tiles); 0 = round 5's shapes
 *   predict.tn_fill (1)   split count of the prediction back contraction (D > 256) chosen so that its units fill whole rounds of the
 *                         chip (0 = round 5's rule: at least three rounds' worth)
 *   nys.syrk_split (1)    Gram matrix K_nm^T K_nm of the Nystroem build cut along the rows into up to 8 partial sums when its tile
 *                         count is only a few rounds of the chip (a tile's k loop is as long as the factor is tall); 0 = one pass
 *   nys.trsm_left (1)     tall triangular solves of the Nystroem build left-looking (one deep product per 512-column strip); 0 = right-looking
 *   chol.nb (512)         panel width of the blocked Cholesky (a multiple of 64 up to 512, anything else falls back to 512)
 *   chol.fused_min_rows (12288)  trailing rows from which a panel's diagonal block is factored inside the trailing-update launch
 *                         (at least 1: a fused launch needs a trailing matrix; smaller values are taken as 1)
 *   chol.outer (1024)     panel pairs: K = 2 nb trailing update in two launches (= chol.nb, or chol.nb not a multiple of 128:
 *                         single panels only)
 *   chol.outer_min_rows (16384)  trailing rows below which new panels are single again
 *   chol.deep (4096)      W > 0 (a multiple of chol.outer): columns in blocks of W; the trailing tiles right of the current block
 *                         receive the block in ONE pass of depth W, which rides in the launches of the next block's outer steps
 *                         (csrc/tile_sched.h: chol_plan_build).  Same factor bit for bit.  0: every outer step updates the
 *                         whole trailing matrix
 *   chol.deep_min_rows (26624)  trailing rows below which the deep schedule hands over to the one-level one
 *   gemm.balance (1)      lower (SYRK-shaped) trailing updates: tile list dealt evenly over the 8 XCDs, no empty workgroups
 *                         (csrc/tile_sched.h); 0: the 8 x 8 super-tile enumeration with 64 block slots per super tile.  Same factor bit for bit
 *   trsm.debug (0)        timing-only ablation mask of the row-local panel solve (results are wrong when set)
 *   trsv.persist (1)      backward substitution as one persistent launch
 *   predict.wave_only (0), predict.mfma (1), predict.mfma_wide (1), predict.fill   prediction kernel choice
 *   predict.fused (1)     gdml_predict with 1-8 host geometries (D <= 256, at most 384 coordinates): ONE launch -- geometries in through the kernel
 *                         arguments, descriptors + contraction + last-workgroup reduction + back-projection, E / F out through
 *                         host-mapped memory (0: descriptor kernel, contraction, epilogue and three copies); predict.fused_rows
 *                         (16) table rows per wavefront, predict.fused_spin (1) completion by polling the kernel's sequence
 *                         number instead of synchronising the stream.  This path records no "predict" phase time
 *   lu.nb (64)            panel width of the LU fallback
 *   comm.force_collectives (0)  issue collectives even for world == 1 without a communicator (tests)
 *   dist.nb (512)         row-block size of the distributed Cholesky (multiple of 128)
 *   dist.lookahead (1 from two ranks on, else 0)  distributed Cholesky: 1 = one panel of look-ahead over three streams (block
 *                         broadcasts on a second communicator); 0 = every step in order on the compute stream
 *   dist.force_panels (0) 1: a one-rank gdml_dist_chol_solve keeps the K = 512 panel schedule of the distributed code instead of
 *                         the single-GPU factorisation it otherwise degenerates to (tests / probes)
 *   nys.force_qr (0)      take the alternative (QR-equivalent) branch of the second Nystroem factorisation (tests)
 *   nys.force_fail (0)    treat the first k attempts of the jitter-stabilised Cholesky of K_mm as failed (tests)
 *   pcg.depth (2)         PCG iterations queued ahead of the host's convergence test / callback (0 = synchronous)
 *   pcg.gemv_plain (0)    preconditioner GEMVs with plain instead of non-temporal loads of the streamed factor (A/B)
 *   pcg.precon_form (2)   application of the Nystroem preconditioner: 0 = stored n x m fp64 factor streamed twice per application
 *                         (the reference's form, iterative.py:120-140); 3 = the factor stored in fp32 plus an m x m Gram
 *                         correction (half the bytes per application; the exact Woodbury inverse on the rounded factor's column
 *                         space: csrc/nystroem.hip); 2 = automatic: 3 once the factor reaches 1 GiB per rank, else 0; 1 = matrix-free
 *                         (two kernel mat-vecs + an m x m matrix; experimental: does not converge at lam = 1e-10, never automatic)
 *   pcg.f32_rows_per (1024), pcg.f32_rw (4)  shape of the fp32 form's two GEMVs: rows per partial sum of X32^T v, rows per
 *                         wavefront of X32 t (A/B)
 *   pcg.f32_gram_rows (2048)  fp32 form: rows per chunk of the compensated Gram sum of the rounded factor
 *   pcg.f32_inplace (1)   fp32 form: the rounded factor overlays the fp64 factor in the matrix buffer (no second n x m buffer; the
 *                         leverage scores are cached first); 0 = a separate fp32 copy beside the fp64 factor (round 5)
 *   predict.hess_generic (0)   1: gdml_predict_hessian keeps F_x in memory instead of registers (the path of N > 157; tests)
 *   predict.hess_chunk_rows (0)  cap on the table rows per chunk of gdml_predict_hessian (0 = sized by memory; tests)
 *   predict.cov_chunk (64)     geometries per pass of gdml_predict_cov / gdml_uncert_cross (their rows of the cross-kernel are 3N n
 *                         doubles each; fewer when free memory is short)
 *   predict.cov_global (0)    1: the cross-kernel keeps its per-permutation vectors in global memory (the path of N > 374; tests)
 *   predict.cov_few_rows (256) most rows 3N B that gdml_predict_cov_few sends through its own solve; 0 = always the batched path of
 *                         gdml_predict_cov; values above GDML_COV_FEW_ROWS count as GDML_COV_FEW_ROWS
 *   predict.cov_few_split_timers (0)  1: under gdml_profile the two per-step kernels of gdml_predict_cov_few are timed one by one
 *                         ("few_diag", "few_upd") instead of the whole solve ("few_solve"); the events slow the solve down
 *   predict.md_fused (1)          gdml_md_run with 1-8 replicas of a molecule with D <= 256: one launch per step (0: the general
 *                         route of three pieces per step)
 *   predict.md_chunk_frames (0)   most recorded frames gdml_md_run and gdml_pimd_run queue between two synchronisations (0 = as
 *                         many as fit into 64 MiB); the results do not depend on it
 *   predict.pimd_tile (0)         coordinates per workgroup of gdml_pimd_run's first kernel: 0 = 64 up to 64 beads and 32 beyond,
 *                         32 = always 32.  The results do not depend on it
 *   predict.relax_fused (1)       gdml_relax_run with 1-8 geometries of a molecule with D <= 256: one launch per evaluation (0: the
 *                         general route of two pieces per evaluation)
 *   predict.relax_chunk_steps (32)  evaluations gdml_relax_run (and gdml_neb_run, gdml_cell_relax_run, gdml_ef_run) queues between
 *                         two synchronisations (the host learns at a chunk's end which replicas froze); the results do not depend on it
 *   predict.vib_chunk (0)         geometries per chunk of gdml_vib_run (0 = as many as keep its Hessians and work matrices under
 *                         256 MiB); steps b to d of that entry do not depend on it.  Also the geometries per slice of an
 *                         evaluation of gdml_ef_run
 *   chol.loo_chunk (64)            training points per pass of gdml_loo (their rows of L^-T are 3N n doubles each; fewer when free
 *                         memory is short).  The results do not depend on it
 *   chol.extend_chunk (64)         points per pass of gdml_factor_extend (their 3N rows are assembled, solved and factored together;
 *                         fewer when free memory is short).  Different values agree to rounding, not bit for bit
 *   chol.remove_chunk (64)         removed points per sweep of gdml_factor_remove; a sweep never takes more than 128 columns
 *                         of L[kept, removed] (the LDS of its kernels).  Different values agree to rounding, not bit for bit
 *   chol.select_chunk (64)         candidates per pass of gdml_select_points' first stage (their rows of the cross-kernel are 3N n
 *                         doubles each; fewer when free memory is short).  The results do not depend on it
 *   chol.select_mem_budget (0)     bytes the retained buffers of gdml_select_points may take; 0 = 90 % of free device memory (tests)
 *   chol.evidence_chunk (64)       training points per pass of gdml_evidence_grad (their rows of L^-T and of A^-1 are 3N n doubles
 *                         each; fewer when free memory is short).  Different values agree to rounding, not bit for bit
 *   chol.evidence_mem_budget (0)   bytes gdml_evidence_grad takes for free when it sizes its second matrix; 0 = what
 *                         gdml_mem_info reports (tests)
 *   chol.evidence_global (0)       1: the contraction kernel of gdml_evidence_grad keeps its per-pair vectors and the tile in
 *                         global memory (the path of descriptors beyond LDS, N > 140 or so; tests)
 *   pcg.f32_min_pivot (1e-7)  fp32 form: smallest squared Cholesky pivot of the rounded factor's Gram matrix below which the
 *                         reference's fp64 form is kept (gdml_get_option("pcg.f32_last_min_pivot") reads the last value seen)
 * Unknown keys return GDML_ERR_INVALID. */
int gdml_set_option(gdml_ctx* ctx, const char* key, double value);
int gdml_get_option(gdml_ctx* ctx, const char* key, double* value_out, int* is_set_out);

/* ---- descriptors  (replaces Desc.from_R, sgdml/utils/desc.py:288-365, :208-239) --------
 * R (M,3N) -> R_desc (M,D) = 1/|r_i - r_j|, R_d_desc (M,D,3) = (r_i - r_j)/d^3.
 * lat / lat_inv: 3x3 row-major lattice (columns = vectors) and its inverse, or both NULL;
 * with a lattice the pair differences are wrapped to the minimum image first
 * (desc.py:44-77, round-half-even like np.around). */
int gdml_desc_from_R(gdml_ctx* ctx, const double* R, int64_t M, int N, const double* lat,
                     const double* lat_inv, double* R_desc_out, double* R_d_desc_out);

/* ---- pairwise atom matching of the symmetry search  (replaces the pool of sgdml/utils/perm.py:200-221 and its worker _bipartite_match_wkr, :53-92;
 * SURVEY.md 8(f)4).  One wavefront per pair i < j of the M geometries: cost[a][b] = -sum_k absv_i[a][k] absv_j[b][k], atoms of
 * different species pushed above every same-species entry, the linear assignment by the shortest-augmenting-path algorithm
 * scipy.optimize.linear_sum_assignment implements, kept when it brings geometry i's distance matrix closer to j's
 * (perm.py:76-89: after < before and not numpy.isclose).
 *   absv (M,N,N): |eigenvectors| of the distance matrices, columns by decreasing eigenvalue, or NULL (computed on the device);
 *   adj (M,N,N): distance matrices;
 *   species (N) int32;  cost_out (M,M): entry (i,j), i < j = the pair's remaining distance (the rest 0);
 *   found_ij (capacity,2), found_perm (capacity,N) int32: the kept assignments, in no particular order; *n_found their number --
 *   if it exceeds `capacity` only the first `capacity` were stored (call again with more room; M (M-1)/2 always suffices). */
/* |eigenvectors| (M,N,N) of M symmetric N x N matrices, columns by decreasing eigenvalue (replaces the per-geometry
 * numpy.linalg.eig of perm.py:183-187): one workgroup per matrix, cyclic two-sided Jacobi in LDS.  gdml_perm_match runs the same
 * kernel when `absv` is NULL.  (gdml_sym_eig below returns eigenvalues and signed eigenvectors from the same sweeps.) */
int gdml_sym_eig_absv(gdml_ctx* ctx, const double* adj, int64_t M, int N, double* absv_out);
int gdml_perm_match(gdml_ctx* ctx, const double* absv, const double* adj, const int32_t* species, int64_t M, int N,
                    double* cost_out, int32_t* found_ij, int32_t* found_perm, int64_t capacity, int64_t* n_found);

/* ---- training set residency (replaces the H2D copies at sgdml/train.py:1447-1448) -------
 * tril_perms is the (P,D) descriptor-permutation table, i.e. the un-linearised form of
 * tril_perms_lin (train.py:897-904): tril_perms[p][k] = tril_perms_lin[k*P+p] - p*D.  Each
 * row must be induced by an atom permutation (Desc.perm, desc.py:509-539); the library
 * recovers the atom permutations and rejects anything else with GDML_ERR_INVALID. */
int gdml_train_upload(gdml_ctx* ctx, const double* R_desc, const double* R_d_desc, int64_t M,
                      int N, const int64_t* tril_perms, int P);

/* ---- kernel matrix assembly (replaces GDMLTrain._assemble_kernel_mat, train.py:1260-1535,
 *      worker train.py:97-302, torch backend torchtools.py:110-392) -----------------------
 * Builds the UN-negated kernel matrix with rows = 3N*M (+M if use_E_cstr) and the selected
 * columns, element order exactly as train.py:1535, into a device buffer owned by the
 * context (it stays there for gdml_chol_factor / gdml_nystroem_*), and optionally copies
 * it to K_host_out (row stride ldk doubles, at least n_cols) when that is not NULL.
 *   col_kind GDML_COLS_ALL    : all columns (col_a, col_b, idx ignored)
 *   col_kind GDML_COLS_POINTS : columns of training points [col_a, col_b)  (whole 3N blocks;
 *                               the reference's slice path train.py:1357-1374)
 *   col_kind GDML_COLS_INDEX  : n_idx sorted unique global column indices idx[] (may include
 *                               energy-constraint columns >= 3N*M; train.py:1376-1407)
 * alloc_extra_rows: extra (uninitialised) rows appended to the device matrix and to the
 * host copy's shape contract (train.py:1418,1484). */
enum { GDML_COLS_ALL = 0, GDML_COLS_POINTS = 1, GDML_COLS_INDEX = 2 };
int gdml_assemble_K(gdml_ctx* ctx, double sig, int use_E_cstr, int col_kind, int64_t col_a,
                    int64_t col_b, const int64_t* idx, int64_t n_idx, int64_t alloc_extra_rows,
                    double* K_host_out, int64_t ldk);

/* Analytic path (Analytic.solve, analytic.py:65-94): the system matrix A = -K + lam I in the form
 * gdml_chol_factor consumes, assembled in one pass -- sign flip (analytic.py:65) and regularisation
 * (analytic.py:82) fused into the stores, and only the blocks on/below the block diagonal written (the
 * factorisation never reads the strict upper triangle): 4 n^2 bytes of HBM traffic instead of 8 n^2 written +
 * 8 n^2 re-read and re-written.  All columns, matrix stays on the device; alloc_extra_rows as above (1 for
 * gdml_chol_set_rhs).  Where the fused form is not available (permutations, energy constraints, N > 21) this is
 * gdml_assemble_K(GDML_COLS_ALL) and gdml_chol_factor applies sign and shift itself.  gdml_chol_factor must be
 * called with the same lam. */
int gdml_assemble_A(gdml_ctx* ctx, double sig, double lam, int use_E_cstr, int64_t alloc_extra_rows);

/* Shape of the device-resident matrix produced by the last gdml_assemble_K. */
int gdml_K_shape(gdml_ctx* ctx, int64_t* n_rows, int64_t* n_cols, int64_t* extra_rows);

/* ---- analytic solve (replaces Analytic.solve, sgdml/solvers/analytic.py:65-99) ----------
 * Requires a square device-resident K from gdml_assemble_K(GDML_COLS_ALL).
 * gdml_chol_factor: A = -K + lam*I, in-place blocked Cholesky A = L L^T on fp64 MFMA.
 *   *info = 0 ok; > 0: leading minor of that order is not positive definite (LAPACK dpotrf
 *   convention, what scipy.linalg.cho_factor raises LinAlgError for, analytic.py:94-101);
 *   the function then returns GDML_ERR_NOT_PD and K is destroyed (re-assemble to retry).
 * gdml_chol_solve: alphas = -(A^-1 y)   (analytic.py:97-99).
 * n_refine > 0 adds that many steps of iterative refinement with the matrix-free kernel
 * operator (needs the training set of gdml_train_upload; 0 = exactly LAPACK semantics).
 * gdml_chol_set_rhs (optional, between gdml_assemble_K(..., alloc_extra_rows >= 1) and
 *   gdml_chol_factor): hands the right-hand side over before the factorisation.  y is carried as an extra
 *   row of the matrix, so the panel solves and trailing updates of the factorisation perform the forward
 *   substitution L z = y on the way (cho_solve's first triangular solve, analytic.py:97, for free);
 *   gdml_chol_solve(y = NULL) then only runs the backward substitution. */
int gdml_chol_set_rhs(gdml_ctx* ctx, const double* y, int64_t n);
/* LU branch of Analytic.solve (analytic.py:101-114: scipy.linalg.solve = LAPACK dgesv, taken when cho_factor
 * raised LinAlgError): needs the FULL un-negated K of gdml_assemble_K(GDML_COLS_ALL) (assemble again after a
 * failed gdml_chol_factor, which destroys the matrix), forms A = -K + lam I on both triangles, factors
 * P A = L U with partial pivoting on the device (blocked, trailing updates on fp64 MFMA) and returns
 * alphas = -(A^-1 y).  *info > 0: U(info,info) is exactly zero (dgetrf convention; scipy raises "Matrix is
 * singular") and the function returns GDML_ERR_NOT_PD.  The matrix is consumed.
 * The least-squares branch (analytic.py:138) only runs for a non-square K, which Analytic.solve never builds. */
int gdml_lu_solve(gdml_ctx* ctx, double lam, const double* y, int64_t n, double* alphas_out, int* info);
int gdml_chol_factor(gdml_ctx* ctx, double lam, int* info);
int gdml_chol_solve(gdml_ctx* ctx, const double* y, int64_t n, int n_refine, double* alphas_out);

/* ---- prediction (replaces GDMLPredict.__init__/set_alphas/predict,
 *      sgdml/predict.py:426-447, :551-601, :1146-1294; worker :84-245; torch :877-1046) ----
 * gdml_predict_upload_model: training descriptors R_desc (M,D) [note: the model file stores
 *   its transpose, train.py:807], R_d_desc_alpha (M,D), tril_perms (P,D), sig, optional
 *   alphas_E (M) (NULL if the model has no energy constraints).  Builds the permuted tables
 *   of predict.py:426-441 on the device.
 * gdml_set_alphas: training-mode re-targeting (predict.py:551-601): needs the Jacobians of
 *   gdml_train_upload; computes J_m alpha_m on the device (desc.py:368-385).
 * gdml_predict: R (B,3N) host geometries, or R == NULL for the training-set mode
 *   (predict.py:1221-1233) which uses the descriptors of gdml_train_upload.  Outputs are
 *   UNSCALED (host applies std and c exactly as predict.py:1286-1288): E_out (B) may be NULL
 *   (return_E=False), F_out (B,3N). */
int gdml_predict_upload_model(gdml_ctx* ctx, const double* R_desc, const double* R_d_desc_alpha,
                              int64_t M, int N, const int64_t* tril_perms, int P, double sig,
                              const double* alphas_E);
int gdml_set_alphas(gdml_ctx* ctx, const double* alphas_F, const double* alphas_E);
int gdml_predict(gdml_ctx* ctx, const double* R, int64_t B, const double* lat,
                 const double* lat_inv, double* E_out, double* F_out);

/* Device-resident variant used by benchmarks and MD loops: R_dev / E_dev / F_dev are DEVICE
 * pointers (hipMalloc'd by the caller or gdml_dev_alloc); nothing crosses PCIe. */
int gdml_predict_dev(gdml_ctx* ctx, const double* R_dev, int64_t B, const double* lat,
                     const double* lat_inv, double* E_dev, double* F_dev);

/* Molecular dynamics on the device: B independent replicas of the model's molecule advance n_steps with positions,
 * velocities and forces resident in device memory; the host sees the recorded frames only.  The reference has no
 * counterpart (its users drive GDMLPredict.predict from ASE, one host round trip per step).
 * With a_i = f_scale F'_i / mass[atom(i)] (F' the library's unscaled force, f_scale = std times the caller's unit factor):
 *   thermostat 0 (NVE, velocity Verlet):  v += dt/2 a(F);  r += dt v;  F = predictor(r);  v += dt/2 a(F)
 *   thermostat 1 (Langevin, BAOAB):       v += dt/2 a(F);  r += dt/2 v;  v = c1 v + c2 sqrt(kT / m) xi;  r += dt/2 v;
 *                                         F = predictor(r);  v += dt/2 a(F)       c1 = exp(-gamma dt), c2 = sqrt(1 - c1^2)
 * Noise: xi are standard normals from a counter-based Philox4x32-10 stream.  Key = (low, high) 32 bits of seed, counter =
 *   (step low, step high, replica, block); the four 32-bit outputs x0..x3 of a block give the normals of coordinates
 *   4 block .. 4 block + 3 through two Box-Muller pairs, u = (x + 0.5) 2^-32: (sqrt(-2 ln u0) cos 2 pi u1, ... sin 2 pi u1)
 *   from (x0, x1) and likewise from (x2, x3).  A value depends on (seed, absolute step, replica, coordinate) only -- not on
 *   B, the grid, chunking or record_every.  The step index of the first step is step0, so a continued run (R, V from the end
 *   of the last one, step0 advanced by its n_steps) draws the continuation of the stream.
 *   gdml_md_noise returns exactly the xi (B,n3) that a Langevin step of index `step` consumes (tests pin the stream with it).
 * Two routes, the same arithmetic of a step on both:
 *   single launch (the shapes of predict.fused: D <= 256, B <= 8; option predict.md_fused): ONE kernel per step, modelled on
 *     the single-launch predictor -- its row loop, row split and reduction order.  The state of step t is read from one half
 *     of a ping-pong buffer; every workgroup of a replica redoes the kick, drift and noise to hold r(t+1); the replica's last
 *     workgroup (ticket) sums the partials in a fixed order, back-projects F(t+1), finishes the velocity, sums the kinetic
 *     energy and writes step t + 1 to the other half and to the frame slot.  The forces of the start geometry come from the
 *     same kernel.  No persistent kernel, no waiting between workgroups, no graph, no host polling;
 *   general (every other shape gdml_predict accepts): an elementwise kernel (kick, drift, noise), the device prediction path
 *     exactly as gdml_predict_dev runs it (same route selection, same kernels) and a second elementwise kernel (kick,
 *     kinetic energy of each replica, frame write).
 *   Steps are plain launches queued back to back on the context's stream.  The host synchronises once per chunk of frames
 *   (at most 64 MiB of frames and 4096 steps; option predict.md_chunk_frames).  The kinetic energy is summed by one fixed
 *   tree on both routes.
 * Frame k is the state after step (k + 1) record_every, n_rec = n_steps / record_every: R_rec, V_rec, F_rec (n_rec,B,3N), each
 *   may be NULL; E_rec (n_rec,B) = E' UNSCALED like gdml_predict, Ekin_rec (n_rec,B) = sum m v^2 / 2.  R and V (B,3N) hold the
 *   start on entry and the end state on return.  lat / lat_inv: minimum image exactly as the predictor applies it; positions
 *   are never wrapped.  first_bad_step (B): absolute index of the first step at which a coordinate, velocity, force or energy
 *   of that replica stopped being finite, -1 = none; checked at every chunk end, the run stops with the chunk.
 * Bit-identical: on the general route E_rec and F_rec of a frame are what gdml_predict_dev returns for that frame's R_rec
 *   (same B; on the single-launch route they agree with gdml_predict to its tolerance); on both routes the same call
 *   repeated; n steps followed by n steps from the end state with step0 + n against 2n steps; any record_every; any chunk size.
 * fp64 throughout, fixed summation orders, no atomics.  A model must be uploaded (GDML_ERR_STATE; no training-set mode).
 * GDML_ERR_INVALID before any launch, message in gdml_last_error (ctx may be NULL for these checks; the text then is that
 *   of gdml_last_error(NULL)): n_steps < 0, record_every < 1, a mass <= 0, dt <= 0, gamma < 0, kT < 0, exactly one of lat /
 *   lat_inv, a thermostat other than 0 or 1, step0 < 0, N different from the model's. */
typedef struct gdml_md_params {
  int64_t B;
  int N;
  double dt;
  const double* mass;    /* (N) */
  double f_scale;        /* acceleration = f_scale * F' / mass */
  const double* lat;
  const double* lat_inv; /* both or neither */
  int thermostat;        /* 0 none, 1 Langevin (BAOAB) */
  double gamma, kT;
  uint64_t seed;
  int64_t step0;
} gdml_md_params;
int gdml_md_run(gdml_ctx* ctx, const gdml_md_params* params, double* R, double* V, int64_t n_steps, int64_t record_every,
                double* R_rec, double* V_rec, double* F_rec, double* E_rec, double* Ekin_rec, int64_t* first_bad_step);
int gdml_md_noise(uint64_t seed, int64_t step, int64_t B, int n3, double* xi_out, gdml_ctx* ctx);

/* Path-integral molecular dynamics on the device: B independent ring polymers of P = beads replicas of the model's molecule
 * (nuclear quantum effects), state (B,P,3N) resident in device memory like gdml_md_run's.  The reference has no counterpart
 * (its users drive i-PI or ASE, one host round trip per bead and step).
 * Hamiltonian, sampled at the bead temperature P kT with omega_P = P kT / hbar (hbar in the caller's units):
 *   H_P = sum_j [ m v_j^2 / 2 + m omega_P^2 (r_j - r_{j+1})^2 / 2 + f_unit E(r_j) ],   r_{P+1} = r_1
 *   every bead feels the full physical force, a_j = f_scale F'(r_j) / mass[atom], exactly as in gdml_md_run.
 * Normal modes: the orthonormal real DFT over the bead index, C[j][k], j, k = 0 .. P-1,
 *   k = 0: 1 / sqrt P;   0 < 2k < P: sqrt(2/P) cos(2 pi j k / P);   2k = P: (-1)^j / sqrt P;   2k > P: sqrt(2/P) sin(2 pi j k / P)
 *   with frequencies omega_k = 2 omega_P sin(k pi / P).  C is built on the host in fp64 and uploaded once per call; the
 *   transform is a dense P x P product per coordinate summed in index order (no FFT: a fixed order keeps runs reproducible);
 *   the internal modes (k > 0, columns that sum to zero) are formed from r_j - r_0 and v_j - v_0, so that nothing cancels
 *   against |r| and a collapsed ring (all beads equal) has internal modes that are exactly zero and stays collapsed under RPMD.
 *   gdml_pimd_modes returns the matrix and frequencies a run uses; it needs neither a context nor a device.
 * One step of absolute index s (BAOAB with the drift replaced by the exact free ring-polymer flow):
 *   v_j += dt/2 a_j;   (q~, v~) = C^T (r, v);   flow;   (r, v) = C (q~, v~);   F = predictor(all B P geometries);   v_j += dt/2 a_j
 *   flow over tau:  q~' = cos(w_k tau) q~ + sin(w_k tau) / w_k v~,  v~' = -w_k sin(w_k tau) q~ + cos(w_k tau) v~  (w_k = 0: q~' = q~ + tau v~)
 *   thermostat 0 (RPMD, microcanonical): one flow with tau = dt, no noise
 *   thermostat 1 (PILE-L): flow dt/2;  v~ = c1_k v~ + c2_k sqrt(P kT / m) xi;  flow dt/2;   c1_k = exp(-gamma_k dt), c2_k = sqrt(1 - c1_k^2),
 *     gamma_0 = gamma_centroid (0: the centroid is not thermostatted, T-RPMD), gamma_k = pile_lambda 2 omega_k for k > 0
 *     (pile_lambda = 1: Ceriotti, Parrinello, Markland, Manolopoulos, J. Chem. Phys. 133, 124104 (2010)).
 * Noise: xi of (ring b, mode k, coordinate c) at step s is gdml_md_run's stream with the replica index b P + k -- drawn in
 *   mode space, a function of (seed, absolute step, ring, mode, coordinate) and of P only.  With P = 1 it is gdml_md_run's.
 * Three pieces per step, stream order the only dependency: a kernel whose workgroups each own all beads of a tile of
 *   coordinates of one ring (kick, transform, flow, thermostat, transform back in LDS; 32 P W bytes for a tile of W = 64
 *   coordinates, W = 32 beyond 64 beads; option predict.pimd_tile = 32 selects the narrow tile for any P, same bits), the
 *   device prediction path as gdml_predict_dev runs it for B P geometries, and a kernel with one workgroup per ring (kick,
 *   centroid, ring quantities, frame write).  Chunks as in gdml_md_run (64 MiB of frames, 4096 steps, predict.md_chunk_frames).
 * R and V (B,P,3N) hold the start on entry and the end state on return.  Frame k is the state after step (k + 1) record_every:
 *   R_rec, V_rec, F_rec (n_rec,B,P,3N), E_rec (n_rec,B,P) = E' of every bead UNSCALED, Rc_rec (n_rec,B,3N) = the bead average
 *   r_c; each may be NULL.  ring_rec (n_rec,B,5), every sum in a fixed order (per-thread partial sums in index order, then
 *   gdml_md_run's 256-slot tree; no floating-point atomics):
 *     [0] E_pot    = (1/P) sum_j E'(r_j)                                   UNSCALED like gdml_predict
 *     [1] E_kin    = sum_j sum m v_j^2 / 2                                 (equipartition: 3N P  P kT / 2)
 *     [2] E_spring = sum_j sum m omega_P^2 (r_j - r_{j+1})^2 / 2
 *     [3] K_cv     = (3N/2) kT - f_scale / (2P) sum_j (r_j - r_c) . F'_j   centroid-virial kinetic-energy estimator
 *     [4] K_prim   = (3N P / 2) kT - E_spring / P                          primitive estimator
 * lat / lat_inv: the predictor's minimum image only; beads are never wrapped.  first_bad_step (B): as in gdml_md_run, per ring;
 *   a ring whose E_kin, E_spring or virial sum overflows counts as non-finite too.
 * Bit-identical: E_rec and F_rec of a frame are what gdml_predict_dev returns for that frame's R_rec as B P geometries; the
 *   same call repeated; n + n continued steps (step0 advanced) against 2n; any record_every, chunk size and tile width.
 * GDML_ERR_INVALID before any launch (ctx may be NULL for these checks): everything gdml_md_run rejects (gamma_centroid < 0
 *   in gamma's place), beads outside 1 .. 128, hbar <= 0 or not finite, kT <= 0 with beads > 1, pile_lambda <= 0,
 *   B beads >= 2^31. */
typedef struct gdml_pimd_params {
  int64_t B;
  int N;
  int beads;
  double dt;
  const double* mass;    /* (N) */
  double f_scale;        /* acceleration = f_scale * F' / mass */
  const double* lat;
  const double* lat_inv; /* both or neither */
  int thermostat;        /* 0 none (RPMD), 1 PILE-L */
  double gamma_centroid, pile_lambda, kT, hbar;
  uint64_t seed;
  int64_t step0;
} gdml_pimd_params;      /* 112 bytes */
int gdml_pimd_run(gdml_ctx* ctx, const gdml_pimd_params* params, double* R, double* V, int64_t n_steps, int64_t record_every,
                  double* R_rec, double* V_rec, double* F_rec, double* E_rec, double* Rc_rec, double* ring_rec,
                  int64_t* first_bad_step);
int gdml_pimd_modes(int beads, double kT, double hbar, double* C /* (P,P) row j, column k */, double* omega /* (P) */);

/* Geometry relaxation on the device: B independent geometries of the model's molecule descend to a minimum of the energy by
 * FIRE (Bitzek, Koskinen, Gaehler, Moseler, Gumbsch, Phys. Rev. Lett. 97, 170201 (2006)) in the form ASE's FIRE optimiser
 * uses: unit masses, the whole 3N-vector step clipped.  Positions, velocities, forces and the optimiser's state stay resident
 * in device memory; the host sees the end state and a small history.  The reference has no counterpart (its users drive
 * GDMLPredict.predict from ASE's optimisers, one host round trip per step).
 * The step.  g = f_scale F' (F' the library's unscaled force, f_scale = std times the caller's unit factor); all sums and
 *   norms run over a replica's 3N coordinates.  Per-replica state: v, dt, alpha, n_pos (steps since the last negative
 *   power), n_taken (steps taken in the replica's lifetime).  Evaluation t = 0, 1, ... of a replica that is still active:
 *   1. E', F' = predictor(r);  f_atom = max over atoms of |g_atom|;  E' and f_atom go into the history.  A non-finite r, v, F'
 *      or E' sets the replica's first_bad_step (to t), as in gdml_md_run; such a replica never counts as converged.
 *   2. f_atom < fmax: the replica is converged.  Its r, v, dt, alpha, n_pos, n_taken, E' and F' freeze: never written again.
 *   3. otherwise, t = max_steps (the budget of this call is used up): the replica stops unconverged and freezes the same way.
 *   4. otherwise update:
 *        if n_taken > 0:  p = g . v
 *          p > 0:   v <- (1 - alpha) v + (alpha |v| / |g|) g;   then, if n_pos > n_min:  dt <- min(dt f_inc, dt_max),
 *                   alpha <- alpha f_alpha;   then n_pos += 1
 *          p <= 0:  v <- 0,  alpha <- alpha_start,  dt <- dt f_dec,  n_pos <- 0
 *        (n_taken = 0 skips this block -- ASE's "v is None" case; without it a fresh start would halve dt at once)
 *        v <- v + dt g;   Delta = dt v;   if |Delta| > max_step:  Delta <- Delta (max_step / |Delta|);   r <- r + Delta;
 *        n_taken += 1
 *   A call makes at most max_steps + 1 evaluations per replica; E_end and F_end are always those of R_end.
 *   Sums (g.v, |g|^2, |v|^2, |Delta|^2): per-thread partial sums in index order (coordinate k, k + 256, ...), then
 *   gdml_md_run's 256-slot tree; the maximum over atoms is order-independent.  No floating-point atomics.
 *   lat / lat_inv: the predictor's minimum image only; positions are never wrapped; the cell is fixed.
 * Two routes, the same arithmetic of an update on both (one device function):
 *   general (any shape): per evaluation the device prediction path exactly as gdml_predict_dev runs it for all B geometries
 *     (frozen ones included; their results are discarded, so a frozen replica keeps the bits of its last evaluation), then a
 *     kernel with one workgroup per replica: reductions, convergence test, update, history and frame write.  It writes
 *     nothing another workgroup reads;
 *   single launch (the shapes of predict.fused: D <= 256, B <= 8; option predict.relax_fused): ONE kernel per evaluation,
 *     modelled on gdml_md_run's -- the predictor's row loop, row split, partial sums and ticket.  The replica's last
 *     workgroup sums the partials in the predictor's order, back-projects F' and does 1-4 above; r(t+1) goes into the other
 *     half of a ping-pong buffer (a freezing replica writes its r there too, so both halves hold it from then on).  The
 *     workgroups of a frozen replica read its status word, written by an earlier launch, and return at once.  No persistent
 *     kernel, no waiting between workgroups, no graph, no host polling.
 *   Evaluations are plain launches queued back to back; the host synchronises once per chunk (option
 *   predict.relax_chunk_steps evaluations, and at most predict.md_chunk_frames frames / 64 MiB when R is recorded), reads
 *   the status words and first_bad_step flags and stops when no replica is active.  Frozen replicas are never rewritten, so
 *   nothing in the result depends on the chunk length.
 * Arguments.  R, V (B,3N), dt, alpha (B), n_pos, n_taken (B, int64): the state, the start on entry and the end on return (a
 *   fresh start: V = 0, dt = the first time step, alpha = alpha_start, n_pos = n_taken = 0).  Passing the end state back
 *   continues the run as if it had not been cut (max_steps is the budget of one call).
 *   status (B,2) int64: [0] = 1 converged, 0 budget used up, -1 still active (only after a non-finite value stopped the
 *   run); [1] = the evaluation of this call at which the replica froze = the steps it took in this call (-1 if active).
 *   With n_made = 1 + the largest status[.][1] (the evaluations made; launches beyond it found every replica frozen):
 *   E_hist, fmax_hist (max_steps + 1, B): rows 0 .. n_made - 1 are written, E' UNSCALED like gdml_predict and f_atom; a frozen
 *   replica repeats its last value.  R_rec (max_steps / record_every + 1, B, 3N) or NULL (then record_every is not used):
 *   frame k = the positions of evaluation k record_every, written for k record_every < n_made, a frozen replica repeating
 *   its end positions.  record_every = 0 is allowed with R_rec = NULL only.  E_end (B), F_end (B,3N): E', F' UNSCALED at R.
 *   first_bad_step (B): evaluation at which a value of the replica stopped being finite, -1 = none; checked at chunk ends.
 * Bit-identical: the same call repeated; n steps then a continuation against 2 n steps; any chunk length; any record_every;
 *   on the general route E_end, F_end are what gdml_predict_dev returns for R (same B).
 * GDML_ERR_INVALID before any launch (ctx may be NULL for these checks): fmax <= 0 or not finite, max_steps < 0, a dt <= 0,
 *   dt_max < a dt, max_step <= 0, f_inc < 1, f_dec outside (0, 1), alpha_start or f_alpha outside (0, 1], n_min < 0,
 *   record_every < 0 (< 1 with R_rec), exactly one of lat / lat_inv, a NULL state or output array, N different from the
 *   model's.  GDML_ERR_STATE without a model. */
typedef struct gdml_relax_params {
  int64_t B;
  int N;
  double f_scale;        /* g = f_scale * F' */
  const double* lat;
  const double* lat_inv; /* both or neither */
  double fmax;           /* converged when the largest |g_atom| is below it */
  double dt_max, max_step;
  double f_inc, f_dec, alpha_start, f_alpha;
  int64_t n_min;
} gdml_relax_params;     /* 104 bytes */
int gdml_relax_run(gdml_ctx* ctx, const gdml_relax_params* params, double* R, double* V, double* dt, double* alpha,
                   int64_t* n_pos, int64_t* n_taken, int64_t max_steps, int64_t record_every, double* R_rec, double* E_hist,
                   double* fmax_hist, double* E_end, double* F_end, int64_t* status, int64_t* first_bad_step);

/* Nudged elastic band on the device: B independent bands of P images each, images 0 and P - 1 fixed end points (two minima),
 * relax to the minimum-energy path between them; with `climb` the highest image climbs to the saddle, whose energy above the
 * end points is the barrier.  A band is ONE FIRE system (one v, dt, alpha, n_pos, n_taken per band), which is how ASE drives
 * FIRE(NEB(...)).  Positions, velocities, forces and the optimiser's state stay resident in device memory.  The reference has
 * no counterpart (its users wrap GDMLPredict.predict in ASE's NEB, one host round trip per evaluation).
 * The step.  g = f_scale F' as in gdml_relax_run; E' is the predictor's unscaled energy.  Evaluation t = 0, 1, ... of a band
 *   that is still active:
 *   1. E', F' = predictor of all P images.  The end points are recomputed each evaluation and their results are not used for
 *      motion (so E_end, F_end are what gdml_predict_dev returns for the B P geometries of R).
 *   2. NEB force.  For every interior image i, with tau+ = r_{i+1} - r_i and tau- = r_i - r_{i-1} (plain differences;
 *      positions are never wrapped), the improved tangent (Henkelman, Jonsson, J. Chem. Phys. 113, 9978 (2000)):
 *        E_{i+1} > E_i > E_{i-1}:  tau = tau+
 *        E_{i+1} < E_i < E_{i-1}:  tau = tau-
 *        otherwise, with dE_max and dE_min the larger and the smaller of |E_{i+1} - E_i| and |E_{i-1} - E_i|:
 *          tau = tau+ dE_max + tau- dE_min  if E_{i+1} > E_{i-1},  else  tau = tau+ dE_min + tau- dE_max
 *        tau^ = tau / |tau|
 *      F_i = g_i - (g_i . tau^) tau^ + k (|tau+| - |tau-|) tau^          (k = k_spring, in units of g per length)
 *      With climb: the interior image of highest E' (ties go to the lowest index; chosen anew at every evaluation) gets
 *      F_i = g_i - 2 (g_i . tau^) tau^ and no spring (Henkelman, Uberuaga, Jonsson, J. Chem. Phys. 113, 9901 (2000)).
 *      Energies enter through comparisons and the ratio of the two dE only: their scale and offset do not matter.
 *   3. Convergence.  f_atom = max over interior images and atoms of |F_{i,atom}|; E'(highest interior image) and f_atom go
 *      into the history.  f_atom < fmax: the band is converged; otherwise t = max_steps: it stops unconverged.  A frozen band
 *      is never written again, exactly as a frozen replica of gdml_relax_run.  A non-finite r, v, F or E' of the band sets
 *      first_bad_step (to t); such a band never counts as converged.
 *   4. Update.  Otherwise gdml_relax_run's update 4, verbatim, on the band vector of (P - 2) 3N coordinates with F in place
 *      of g (the n_taken = 0 case, the clip of the whole vector to max_step and the counters included).
 *   Sums: the four per-image sums (g . tau, |tau+|^2, |tau-|^2, |tau|^2) over 3N and the band sums (F . v, |F|^2, |v|^2,
 *   |Delta|^2) over (P - 2) 3N as per-thread partial sums in index order (k, k + 256, ...), then gdml_md_run's 256-slot tree.
 *   No floating-point atomics.
 * Three pieces per evaluation, stream order the only dependency: the device prediction path for the B P geometries exactly
 *   as gdml_predict_dev runs it; neb_force_kernel, one workgroup per interior image (it finds the climbing image itself from
 *   the band's energies and writes nothing another workgroup of the launch reads); neb_step_kernel, one workgroup per band:
 *   gdml_relax_run's update function on the band vector, history, frame and status, and on freeze the end-of-run outputs.
 *   Workgroups of a frozen band read its status word and return at once.  Chunks, readback and the recorder are
 *   gdml_relax_run's (predict.relax_chunk_steps, predict.md_chunk_frames / 64 MiB); nothing depends on the chunk length.
 * Arguments.  R, V (B,P,3N), dt, alpha (B), n_pos, n_taken (B, int64): the state, start on entry and end on return; rows 0 and
 *   P - 1 of every band of R and V are never written (pass V = 0 there).  Passing the end state back continues the run as if
 *   it had not been cut; a relaxation without climb followed by one with climb is such a continuation.
 *   status, first_bad_step, record_every: as in gdml_relax_run, per band.  Emax_hist, fmax_hist (max_steps + 1, B): E'
 *   UNSCALED of the highest interior image, and f_atom, of the evaluations made.  R_rec (max_steps / record_every + 1, B, P,
 *   3N) or NULL.  Written when a band freezes (zero for a band that a non-finite value stopped): E_end (B,P), F_end (B,P,3N):
 *   E', F' UNSCALED at R;  i_climb (B): the interior image of highest E';  s (B,P): cumulative Euclidean arc length
 *   sum_{j<=i} |r_j - r_{j-1}|;  f_tangent (B,P): g . tau^ of the interior images, 0 at the ends.
 * Bit-identical: the same call repeated; n steps then a continuation against 2 n steps; any chunk length; any record_every.
 * GDML_ERR_INVALID before any launch (ctx may be NULL for these checks): everything gdml_relax_run rejects, P outside
 *   3 ... 128, k_spring <= 0 or not finite, B P >= 2^31, a NULL state or output array.  GDML_ERR_STATE without a model. */
typedef struct gdml_neb_params {
  int64_t B;             /* bands */
  int N;
  int P;                 /* images per band, end points included */
  double f_scale;        /* g = f_scale * F' */
  const double* lat;
  const double* lat_inv; /* both or neither */
  double fmax;           /* converged when the largest |F_atom| of the interior images is below it */
  double dt_max, max_step;
  double f_inc, f_dec, alpha_start, f_alpha;
  int64_t n_min;
  double k_spring;
  int climb;             /* 0: plain band, else the highest image climbs */
} gdml_neb_params;       /* 120 bytes */
int gdml_neb_run(gdml_ctx* ctx, const gdml_neb_params* params, double* R, double* V, double* dt, double* alpha, int64_t* n_pos,
                 int64_t* n_taken, int64_t max_steps, int64_t record_every, double* R_rec, double* Emax_hist, double* fmax_hist,
                 double* E_end, double* F_end, int64_t* i_climb, double* s, double* f_tangent, int64_t* status,
                 int64_t* first_bad_step);

/* Strain derivative (virial) of B geometries: what pressure, NPT dynamics, cell relaxation and equation-of-state scans of a
 * periodic model need, and what its forces cannot give (with minimum-image pair vectors sum_i f_i (x) r_i is not the strain
 * derivative).  The reference has no counterpart.  Straining atoms and cell together, r -> (I + eps) r, lattice -> (I + eps)
 * lattice, leaves the minimum-image integers as they are, so with the descriptor-space gradient F_x of the predictor
 * (F = J_x^T F_x), d_k the minimum-image pair vector of descriptor entry k, x_k = 1 / |d_k| and g_k = d_k / |d_k|^3:
 *   W = dE' / d eps = sum_k F_x[k] g_k (x) d_k        (symmetric 3 x 3; stress = std W / |det lattice|, +dE/d eps: ASE's sign)
 * Outputs are UNSCALED like gdml_predict (the caller multiplies by std): E_out (B) = E', F_out (B,3N) = F (both may be NULL)
 * and bit-identical to gdml_predict's for the same input on the same route, W_out (B,3,3) row-major, both triangles written.
 * R may not be NULL (no training-set mode); lat / lat_inv both or neither -- without a lattice W is still defined and equals
 * -sum_i f_i (x) r_i.  One to eight host geometries (the shapes of predict.fused) stay ONE launch without a copy: W follows F
 * in the host-mapped block.  Every other route ends in an epilogue that sums W next to the back-projection (d_k = g_k / x_k^3
 * from the query tables).  fp64 throughout, fixed reduction trees, no atomics: the same input on the same context gives
 * bit-identical results, and the _dev variant (device pointers throughout) equals the host one on the same route. */
int gdml_predict_virial(gdml_ctx* ctx, const double* R, int64_t B, const double* lat, const double* lat_inv,
                        double* E_out, double* F_out, double* W_out);
int gdml_predict_virial_dev(gdml_ctx* ctx, const double* R_dev, int64_t B, const double* lat,
                            const double* lat_inv, double* E_dev, double* F_dev, double* W_dev);

/* The same prediction with ONE LATTICE PER GEOMETRY: B independent cells, or the B volumes of an equation-of-state scan, as
 * one batch.  lats, lat_invs (B,3,3): geometry b's lattice and its inverse, each row-major with the cell vectors in the
 * COLUMNS like lat everywhere else; both are required (GDML_ERR_INVALID before any launch for a NULL R, lats or lat_invs;
 * there is no training-set mode).  The inverse only feeds the rounding to the minimum image, as in every other entry.
 * Outputs are UNSCALED: E_out (B), F_out (B,3N), W_out (B,3,3) as in gdml_predict_virial; E_out and F_out may be NULL.  W_out
 * may be NULL as well (F_out then may not): the call is then a plain prediction with per-geometry lattices and runs
 * gdml_predict's epilogue.
 * On the general prediction route the lattice enters the descriptor kernel only; every route kernel (WAVE, BIG, BULK, MFMA,
 * WIDE) and both epilogues work from the query tables.  So this entry runs desc_cells_kernel -- desc_kernel with geometry m
 * reading lattice m from device memory, the minimum-image arithmetic being one shared device function -- and everything
 * behind it unchanged: with B equal lattices E, F and W are bit-identical to gdml_predict_virial_dev (W_out = NULL:
 * gdml_predict_dev) with that lattice, and row b of a call with distinct lattices equals row b of the one-lattice call on
 * the whole batch with lattice b.  The host entry ALWAYS takes the general route, for one to eight geometries too: the
 * single-launch predictor holds one lattice by value in its kernel argument.  Hence the host entry equals the _dev entry
 * (device pointers throughout, lattices included) bit for bit, and the same call repeated gives the same bits. */
int gdml_predict_virial_cells(gdml_ctx* ctx, const double* R, int64_t B, const double* lats, const double* lat_invs,
                              double* E_out, double* F_out, double* W_out);
int gdml_predict_virial_cells_dev(gdml_ctx* ctx, const double* R_dev, int64_t B, const double* lats_dev,
                                  const double* lat_invs_dev, double* E_dev, double* F_dev, double* W_dev);

/* Variable-cell relaxation on the device: B independent periodic geometries relax atoms AND cell by FIRE, the whole state
 * resident in device memory -- the equilibrium cell of a periodic model, its volume under pressure, an E(V) curve.  The model
 * users know is ASE's FIRE(UnitCellFilter(atoms)); the reference has no counterpart.
 * State.  Per geometry a fixed reference lattice L0, a deformation gradient Fd (3 x 3) and reference positions s_i, with
 *   r_i = Fd s_i and lattice L = Fd L0 (cell vectors in the columns).  The generalised coordinates are the (N + 3) x 3 array
 *   u = (s_1 ... s_N, C), C = cell_factor Fd (row-major; cell_factor makes the cell rows commensurate with atom rows, ASE
 *   uses N).  ONE FIRE system per geometry over its 3N + 9 coordinates: v, dt, alpha, n_pos, n_taken as in gdml_relax_run.
 *   A fresh start: s = R0, C = cell_factor I, v = 0.
 * Evaluation t = 0, 1, ... of an active geometry:
 *   1. Fd = C / cell_factor (entry by entry);  L = Fd L0;  r_i = Fd s_i;  Vol = |det L|.  All 3 x 3 algebra in fp64 WITHOUT
 *      fused multiply-adds, every product sum from left to right: (A B)_ab = A_a0 B_0b + A_a1 B_1b + A_a2 B_2b.  Inverses by
 *      the adjugate, for M = ((a,b,c),(d,e,f),(g,h,i)):  adj = (ei - fh, ch - bi, bf - ce;  fg - di, ai - cg, cd - af;
 *      dh - eg, bg - ah, ae - bd),  det = a adj_00 + b adj_10 + c adj_20,  M^-1 = adj / det entry by entry.  A non-finite or
 *      zero det L counts as a non-finite value of the geometry (first_bad_step).
 *   2. E', F', W' = gdml_predict_virial_cells_dev for (r, L, L^-1) of all B geometries in one call (frozen ones included;
 *      their results are discarded).
 *   3. Generalised force in the caller's units, g = f_scale F':
 *        G_i = Fd^T g_i;   T = mask o (f_scale W' + pressure Vol I);   G_cell = -T Fd^-T / cell_factor
 *      mask: symmetric 3 x 3 of 0/1 (NULL: all ones) selecting the strain components that relax (in-plane only for a slab:
 *      ones in the upper left 2 x 2).  With mask = 1, G = -dH/du of H = f_scale E' + pressure Vol (dE' = W' : dFd Fd^-1 and
 *      dVol = Vol tr(dFd Fd^-1) at fixed s).
 *   4. f_atom = max over the N + 3 rows of |G_row|.  E', Vol and f_atom go into the history.  Converged (f_atom < fmax),
 *      budget (t = max_steps) and non-finite handling and freezing: gdml_relax_run's steps 1-3; the non-finite check covers
 *      s, C, v, G (hence F' and W'), E' and det L.
 *   5. otherwise gdml_relax_run's update 4, verbatim (the same device function), on u with G, over 3N + 9 coordinates.
 * Launches per evaluation: the prediction (desc_cells_kernel, the route's kernels, the virial epilogue), then ONE kernel with
 *   a workgroup of 256 per geometry: G, the FIRE update, the Cartesian r(t+1), L(t+1), L^-1(t+1) that the next prediction
 *   reads, history, frame, and the end-of-run outputs.  One small launch before evaluation 0 makes r, L, L^-1 of the start.
 *   Sums as in gdml_relax_run (per-thread partial sums in index order, the 256-slot tree); no floating-point atomics.  A
 *   frozen geometry's workgroup returns on its status word; nothing of it is written again.  Chunks, recorder, status and
 *   first_bad_step readback are gdml_relax_run's (predict.relax_chunk_steps, predict.md_chunk_frames / 64 MiB).  There is NO
 *   single-launch route: the single-launch predictor holds one lattice by value in its kernel argument (FusedModel).
 * Arguments.  S (B,3N), Cc (B,3,3), V (B,3N+9), dt, alpha (B), n_pos, n_taken (B, int64): the state, start on entry, end on
 *   return; L0 (B,3,3) is read only.  Passing the end state back with the same L0 continues the run bit for bit.
 *   R_end (B,3N), lat_end (B,3,3): Cartesian end positions Fd s and end lattice Fd L0.  E_end (B), F_end (B,3N), W_end
 *   (B,3,3): UNSCALED, the bits of gdml_predict_virial_cells_dev(R_end, lat_end) at the same B.  vol_end (B) = |det lat_end|.
 *   E_hist, vol_hist, fmax_hist (max_steps + 1, B), status (B,2), first_bad_step (B), record_every: as in gdml_relax_run.
 *   R_rec (max_steps / record_every + 1, B, 3N), lat_rec (.., B, 3, 3): Cartesian frames; each may be NULL.
 * Bit-identical: the same call repeated; n steps then a continuation against 2 n steps; any chunk length; any record_every.
 *   With mask = 0, pressure = 0 and C = cell_factor I: gdml_relax_run's general route with lat = L0 (r = I s is exact and the
 *   zero cell rows add exact zeros to every sum).
 * GDML_ERR_INVALID before any launch (ctx may be NULL for these checks): everything gdml_relax_run rejects; a NULL L0 (a
 *   cell relaxation needs a lattice per geometry), Cc or output array; an L0 or C that is not finite or singular (|det| at
 *   most 1e-12 of the cube of its largest entry); mask entries other than 0 and 1 or an asymmetric mask; cell_factor <= 0 or
 *   not finite; a non-finite pressure.  GDML_ERR_STATE without a model.
 * Not offered: hydrostatic-only and constant-volume modes, the exponential (Frechet) cell parametrisation, L-BFGS.  (Dynamics at
 *   a pressure: gdml_npt_run.) */
typedef struct gdml_cell_relax_params {
  int64_t B;
  int N;
  double f_scale;        /* g = f_scale * F', T = f_scale * W' + pressure Vol */
  double fmax;           /* converged when the largest |G_row| is below it */
  double dt_max, max_step;
  double f_inc, f_dec, alpha_start, f_alpha;
  int64_t n_min;
  double pressure;       /* in units of (f_scale E') per length^3 */
  double cell_factor;    /* C = cell_factor Fd */
  const double* mask;    /* (3,3) of 0/1, symmetric; NULL = all ones */
} gdml_cell_relax_params; /* 112 bytes */
int gdml_cell_relax_run(gdml_ctx* ctx, const gdml_cell_relax_params* params, double* S, double* Cc, const double* L0, double* V,
                        double* dt, double* alpha, int64_t* n_pos, int64_t* n_taken, int64_t max_steps, int64_t record_every,
                        double* R_rec, double* lat_rec, double* E_hist, double* vol_hist, double* fmax_hist, double* R_end,
                        double* lat_end, double* E_end, double* F_end, double* W_end, double* vol_end, int64_t* status,
                        int64_t* first_bad_step);

/* Constant-pressure molecular dynamics on the device: B independent replicas of a PERIODIC model under the isotropic
 * Martyna-Tobias-Klein (MTK) equations -- density, thermal expansion, compressibility.  Positions, velocities, forces, virial,
 * the log-scale eps of the cell and the piston momentum p_eps stay resident in device memory; the host sees recorded frames
 * only.  Two modes: NPH (thermostat 0; no thermostat, piston undamped; it has a conserved quantity) and NPT (thermostat 1;
 * Langevin on the particles and on the piston, a Langevin piston; samples the isothermal-isobaric ensemble).  The model users
 * know is ASE's NPT around a calculator, one host round trip and one stress prediction per replica and step.
 * Per replica:
 *   - the masses are m, N_f = 3N and kappa = 1 + 3/N_f;
 *   - f = f_scale F' and Wv = f_scale W', the library's unscaled force and strain derivative (gdml_predict_virial), with
 *     f_scale = std times the caller's unit factor;  K = sum m v^2 / 2;
 *   - the reference lattice is L0 with inverse L0^-1 and V0 = |det L0|;  the state is (r, v, eps, p_eps);
 *   - the cell is lambda = exp(eps), L = lambda L0, L^-1 = L0^-1 / lambda (entry by entry) and Vol = lambda^3 V0; eps = 0 gives
 *     L0's bits exactly;
 *   - the piston has mass Wp and rate alpha = p_eps / Wp.  Wp = +inf is allowed and makes alpha exactly 0;
 *   - G_eps = kappa 2K - tr(Wv) - 3 P_ext Vol.
 * Step t, with step = step0 + t:
 *   1. p_eps += dt/2 G_eps, from the K, tr Wv and Vol of the current state.
 *   2. alpha = p_eps / Wp and s = exp(-kappa alpha dt/4).  Then v <- s v, v <- v + dt/2 f/m, v <- s v.
 *   3. The drift depends on the thermostat.
 *      No thermostat: q = exp(alpha dt/2).  Then r <- q r, r <- r + dt v, r <- q r, and eps += alpha dt.
 *      Langevin:      q = exp(alpha dt/4).  Then r <- q r, r <- r + dt/2 v, r <- q r, and eps += alpha dt/2.
 *                     v <- c1 v + c2 sqrt(kT/m) xi_k and p_eps <- b1 p_eps + b2 sqrt(Wp kT) xi_3N, with alpha = p_eps / Wp
 *                     afterwards.  The same half drift again with the new alpha.
 *                     c1 = exp(-gamma dt), c2 = sqrt(1 - c1^2);  b1 = exp(-gamma_baro dt), b2 = sqrt(1 - b1^2).
 *                     xi_k is gdml_md_run's stream at (seed, step, replica, coordinate k), k < 3N.  The piston takes
 *                     coordinate index 3N of the same replica.  The particle noise is therefore gdml_md_run's, and
 *                     gdml_md_noise(seed, step, B, 3N + 1) returns everything a step consumes.
 *                     With Wp = inf, b2 sqrt(Wp kT) is not evaluated: the piston is not thermostatted, p_eps stays finite.
 *   4. E', F', W' = gdml_predict_virial_cells_dev(r, L, L^-1) for all B replicas.
 *   5. s = exp(-kappa alpha dt/4) with the current alpha.  Then v <- s v, v <- v + dt/2 f/m, v <- s v.
 *   6. K is summed by gdml_md_run's tree.  Then p_eps += dt/2 G_eps.
 * A frame holds the state after step 6.  Every scaling and kick is the exact flow of one term.  Within each half step every
 * scaling uses the same alpha, so the phase-space volume (r, p, Vol, p_eps) is preserved.  The scheme is symmetric and second
 * order.  In NPH the conserved quantity is H = K + f_unit E + P_ext Vol + p_eps^2 / (2 Wp)  (f_unit E = f_scale E' + const).
 * Launches per step: npt_pre_kernel (one workgroup of 256 per replica; steps 1-3; writes r, v, eps, p_eps and the replica's L
 *   and L^-1 for the predictor), the prediction exactly as gdml_predict_virial_cells_dev runs it, npt_post_kernel (one workgroup
 *   per replica; steps 5-6, the non-finite check and the frame write).  Forces and virial of the start state come from the
 *   same predictor call before step 0, K of the start from the same tree: a continued run starts from the bits its
 *   predecessor ended with.  There is NO single-launch route (the single-launch predictor holds one lattice by value).  Chunks
 *   as in gdml_md_run (64 MiB of frames, 4096 steps, predict.md_chunk_frames).  fp64 throughout, fixed summation orders, no
 *   floating-point atomics; kicks, drifts and the Ornstein-Uhlenbeck step are written with the fused multiply-adds of
 *   gdml_md_run's kernels and nothing else is contracted.
 * Arguments.  R, V (B,3N), eps, p_eps (B): the start state on entry, the end state on return.  L0, L0_inv (B,3,3): reference
 *   lattices (cell vectors in the columns) and their inverses, both required, read only.  Frame k is the state after step
 *   (k + 1) record_every, n_rec = n_steps / record_every: R_rec, V_rec, F_rec (n_rec,B,3N; F' unscaled), lat_rec (n_rec,B,3,3),
 *   each may be NULL; E_rec (n_rec,B) = E' UNSCALED like gdml_md_run's, Ekin_rec = K, vol_rec = Vol, press_rec = P_int =
 *   (2K - tr Wv) / (3 Vol), peps_rec = p_eps.  first_bad_step (B): as in gdml_md_run; it additionally trips on a non-finite
 *   eps, p_eps or Vol.  n_steps = 0 returns the start state untouched.
 * Bit-identical: the same call repeated; n steps followed by n steps from the end state with step0 + n against 2n steps; any
 *   record_every; any chunk size; E_rec and F_rec of a frame are gdml_predict_virial_cells_dev's for that frame's R_rec and
 *   lat_rec at the same B.  With Wp = inf and eps = 0 (any pressure): R, V, F, E', K of gdml_md_run's general route
 *   (predict.md_fused = 0) with lat = L0.
 * GDML_ERR_INVALID before any launch (ctx may be NULL for these checks): everything gdml_md_run rejects; a NULL eps, p_eps, L0
 *   or L0_inv; piston_mass <= 0 or NaN; gamma_baro < 0; a non-finite pressure.  GDML_ERR_STATE without a model.
 * Not offered: anisotropic or fully flexible cells, per-replica pressures, a single-launch route, removal of the centre-of-mass
 *   momentum (N_f = 3N is deliberate), a barostat for gdml_pimd_run. */
typedef struct gdml_npt_params {
  int64_t B;
  int N;
  double dt;
  const double* mass;    /* (N) */
  double f_scale;        /* f = f_scale * F', Wv = f_scale * W' */
  int thermostat;        /* 0 none (NPH), 1 Langevin particles and piston (NPT) */
  double gamma, gamma_baro, kT;
  uint64_t seed;
  int64_t step0;
  double pressure;       /* P_ext, in units of (f_scale E') per length^3 */
  double piston_mass;    /* Wp > 0; +inf freezes the cell */
} gdml_npt_params; /* 104 bytes */
int gdml_npt_run(gdml_ctx* ctx, const gdml_npt_params* params, double* R, double* V, double* eps, double* p_eps,
                 const double* L0, const double* L0_inv, int64_t n_steps, int64_t record_every, double* R_rec, double* V_rec,
                 double* F_rec, double* lat_rec, double* E_rec, double* Ekin_rec, double* vol_rec, double* press_rec,
                 double* peps_rec, int64_t* first_bad_step);

/* Analytic Hessians (force constants) H' = d^2 E' / dR^2 of B geometries, unscaled like gdml_predict (the caller
 * multiplies by std).  The reference has no counterpart: its users take finite differences of predict().
 * With the predictor's per-row quantities (d = x - X_rho, n = sqrt5 |d|, b = 5/(3 sig^3) exp(-n/sig), a = d . v_rho,
 * e_rho = alphas_E entry or 0), u = J_x^T d and w = J_x^T v_rho:
 *   H' = sum_rho [ gam u u^T + s (w u^T + u w^T) ] + tau J_x^T J_x - sum_k F_x[k] grad^2_R x_k
 *   s = -(5/sig) b, gam = 25 a b / (sig^2 n) + (5/sig) e_rho b, tau = sum_rho [ -(5/sig) a b - e_rho b (n + sig) ]
 * (csrc/predict_hess.hip has the derivation's symbols and the kernels).  Outputs: E_out (B) = E', F_out (B,3N) = F (both
 * may be NULL), H_out (B,3N,3N) row-major, coordinate index 3 atom + axis, both triangles written (H is symmetric).
 * R may not be NULL (no training-set mode); lat / lat_inv both or neither.  fp64 throughout, no atomics: the same input on
 * the same context gives bit-identical results, and the _dev variant (device pointers throughout) equals the host one.
 * Molecules up to N = 197; larger ones return GDML_ERR_UNSUPPORTED. */
int gdml_predict_hessian(gdml_ctx* ctx, const double* R, int64_t B, const double* lat, const double* lat_inv,
                         double* E_out, double* F_out, double* H_out);
int gdml_predict_hessian_dev(gdml_ctx* ctx, const double* R_dev, int64_t B, const double* lat,
                             const double* lat_inv, double* E_dev, double* F_dev, double* H_dev);

/* Eigenvalues and eigenvectors of M symmetric n x n matrices on the device: one workgroup per matrix (grid-stride over M),
 * cyclic two-sided Jacobi with the round-robin ordering -- the sweep loop of gdml_sym_eig_absv (csrc/sym_eig.hip; csrc/sym_eig.h holds the one
 * copy both kernels call).  Only the mean of the two triangles of A enters.
 *   w (M,n): eigenvalues ascending; equal ones in the order of their Jacobi columns.
 *   V (M,n,n) or NULL: V[m][k][:] is the unit eigenvector of w[m][k], a ROW; its component of largest magnitude is positive
 *   (the lowest index on ties), so outputs are comparable across calls.  NULL: the same w, bit for bit.
 *   sweeps (M) or NULL: sweeps made per matrix (0 for a diagonal matrix).
 * Storage: working matrix and rotations in LDS when both fit (n <= 100), only the matrix (n <= 141), both in device memory
 *   above that.  A sweep stops the iteration when the off-diagonal mass is below 1e-30 of the whole; at most 30 sweeps.  A
 *   matrix still above the threshold after them (in practice: one that is not finite) makes the call return GDML_ERR_INVALID
 *   naming the first such matrix, after the outputs of all matrices were written.
 * The _dev variant takes device pointers throughout (V_dev may be A_dev: every matrix is read whole before its rows are
 *   written) and synchronises once, to read the sweeps.  The same input gives bit-identical results: on either entry, alone or
 *   inside a batch, with or without V.
 * GDML_ERR_INVALID before any launch (ctx may be NULL for these checks): M < 0, n < 1 or n > 591 (3 x 197), NULL A or w,
 *   M n n >= 2^62.  M = 0 does nothing. */
int gdml_sym_eig(gdml_ctx* ctx, const double* A, int64_t M, int n, double* w, double* V, int64_t* sweeps);
int gdml_sym_eig_dev(gdml_ctx* ctx, const double* A_dev, int64_t M, int n, double* w_dev, double* V_dev, int64_t* sweeps_dev);

/* Harmonic vibrational analysis of B geometries on the device: squared frequencies and normal modes of the mass-weighted
 * Hessian with the rigid-body motion projected out -- what follows gdml_relax_run (is it a minimum?) and gdml_neb_run with a
 * climbing image (is it a first-order saddle?).  The reference has no counterpart.  Per chunk of geometries:
 *   a. H' = gdml_predict_hessian_dev of the chunk; E (B) and F (B,3N) are its E' and F, UNSCALED like gdml_predict (either may
 *      be NULL).
 *   b. D_ij = h_scale sym(H')_ij / sqrt(m_i m_j) (h_scale = std times the caller's unit factor, as f_scale of gdml_md_run).
 *      Rigid basis in mass-weighted coordinates, in this order: translations sqrt(m_i) e_c (project >= 1), infinitesimal
 *      rotations about the centre of mass sqrt(m_i) (e_c x (r_i - r_cm)) (project = 2), c = x, y, z; modified Gram-Schmidt in
 *      that order; a vector whose remainder has a squared norm below 1e-10 of its own is dropped (linear molecule: n_rigid = 5,
 *      one atom: 3).  With Q the orthonormal rows kept and P = I - Q^T Q:
 *        D_s = P D P + Lambda Q^T Q,  Lambda = 2 |P D P|_F (1 if that is 0)
 *      The rigid modes are exact eigenvectors at Lambda and every vibration has |lambda| <= |P D P|_2 < Lambda: a soft or
 *      imaginary vibration is never confused with a rigid mode, however far the geometry is from a stationary point.
 *   c. gdml_sym_eig_dev's kernel on D_s, in place.
 *   d. w2 (B,3N): entries [0, 3N - n_rigid) are the vibrational omega^2 ascending (imaginary modes negative, first); the last
 *      n_rigid entries are exactly 0.  n_neg (B): vibrational entries below -tau, tau = 3N eps |D_s|_F.  modes (B,3N,3N) or
 *      NULL: modes[b][k][:] is the mass-weighted orthonormal vector of w2[b][k]; the last n_rigid rows span the rigid space.
 *      NULL: nothing of size (3N)^2 leaves the device.  sweeps (B) or NULL: Jacobi sweeps per geometry.
 * One workgroup per geometry in b and c, every sum in a fixed order, no atomics.  Chunks hold as many geometries as keep the
 *   Hessians and the eigensolver's work matrices under 256 MiB (option predict.vib_chunk, 0 = automatic; tests).
 * Bit-identical: the same call repeated; modes NULL or not; and steps b to d never depend on the batch or the chunk -- so any
 *   chunk length, and a geometry alone against the same geometry inside a batch, as far as gdml_predict_hessian_dev returns the
 *   same bits for that geometry (its plan depends on the number of geometries per call for large tables).
 * GDML_ERR_INVALID before any launch (ctx may be NULL for these checks): B < 0, N < 1, project outside 0 .. 2, exactly one of
 *   lat / lat_inv, project = 2 with a lattice (rotations are no symmetry of a periodic cell), h_scale not finite or <= 0, a mass
 *   not finite or <= 0, a coordinate that is not finite, NULL params, R, masses, w2, n_rigid or n_neg; N different from the
 *   model's.  GDML_ERR_UNSUPPORTED for N > 197 (the Hessian's limit).  GDML_ERR_STATE without a model. */
typedef struct gdml_vib_params {
  int64_t B;
  int N;
  double h_scale;        /* D = h_scale * M^-1/2 H' M^-1/2 */
  const double* lat;
  const double* lat_inv; /* both or neither */
  int project;           /* 0 none, 1 translations, 2 translations + rotations */
} gdml_vib_params;       /* 48 bytes */
int gdml_vib_run(gdml_ctx* ctx, const gdml_vib_params* params, const double* R, const double* masses, double* w2,
                 double* modes /* or NULL */, int64_t* n_rigid, int64_t* n_neg, double* E, double* F, int64_t* sweeps);

/* Eigenvector following on the device: B independent geometries of the model's molecule move to a stationary point of the
 * energy -- a minimum (order = 0) or a first-order saddle (order = 1) -- by quasi-Newton steps in the eigenbasis of the analytic
 * Hessian (Cerjan, Miller, J. Chem. Phys. 75, 2800 (1981); Baker, J. Comput. Chem. 7, 385 (1986); the per-mode rational-function
 * step in closed form), with a trust radius and mode tracking.  What follows gdml_neb_run with a climbing image (its saddle,
 * tightened to any force threshold) and gdml_relax_run (quadratic convergence near the minimum).  Cartesian coordinates and
 * unit masses, as in gdml_relax_run.  Positions, the state and the Hessians stay resident in device memory.  The reference has
 * no counterpart.
 * One evaluation t = 0, 1, ... of a geometry that is still active.  g = -f_scale F' (f_scale = std times the caller's unit factor):
 *   1. E', F', H' = gdml_predict_hessian_dev of all B geometries (frozen ones included; their results are discarded).
 *   2. gdml_vib_run's step b with unit masses and h_scale = f_scale: D_s = P D P + Lambda Q^T Q (project as there).
 *   3. gdml_sym_eig_dev's kernel on D_s: w ascending, v_i as rows.  The top n_rigid pairs are the rigid modes at Lambda; the
 *      first nv = 3N - n_rigid pairs are the vibrational set, the only ones the step uses.  n_neg and tau as in gdml_vib_run.
 *   4. One kernel, one workgroup of 256 threads per geometry:
 *      a. f_atom = the largest atomic |g|.  E' and f_atom go into the history.  A non-finite r, F', E' or eigenvalue sets
 *         first_bad_step (to t), as does a matrix the Jacobi loop cannot finish; such a geometry never counts as converged.
 *      d. Followed mode k (order = 1): 0 without a follow vector t, else argmax_i |v_i . t| over i < nv, ties to the lowest i.
 *         order = 0: k = 0.  w_follow_hist records w_k, k_follow_hist k.  E_end, F_end, w_end, n_rigid, n_neg and mode_end
 *         (v_k; zeros for order = 0) take this evaluation's values.
 *         f_atom < fmax: converged.  Otherwise t = max_steps: the budget of this call is used up.  Either way the geometry
 *         freezes: R, t, trust, E_prev, dE_pred, flags and the outputs above are never written again (the state is the one this
 *         evaluation started from, so a continuation repeats this evaluation and goes on).
 *      b. Trust update, when flags bit 0 is set and |dE_pred| > 1e-8 max(|E'|, |E_prev|) f_scale (below that the ratio is the
 *         predictor's rounding noise): rho = f_scale (E' - E_prev) / dE_pred;  rho < 0.25 or rho > 1.75: trust <- max(trust / 2,
 *         trust_min);  0.75 < rho < 1.25 and bit 1 set: trust <- min(2 trust, trust_max).  No step is ever rejected.
 *      c. gt_i = v_i . g for i < nv.
 *      e. d_i = |w_i| + sqrt(w_i^2 + 4 gt_i^2);  s_i = -2 gt_i / d_i for a minimised mode, +2 gt_i / d_i for the maximised mode
 *         k (order = 1), 0 when d_i = 0: Newton's step where the curvature has the wanted sign and the gradient is small, a
 *         step along the right side of the gradient where it has not.
 *      f. |s|_2 > trust: s <- s (trust / |s|_2), bit 1 set; otherwise bit 1 cleared.
 *      g. dE_pred <- sum_i gt_i s_i + w_i s_i^2 / 2 (the scaled s);  E_prev <- E';  bit 0 set;  R <- R + sum_i s_i v_i;
 *         t <- v_k (order = 1 with a follow vector).
 *   Sums over modes: per-thread partial sums in index order (mode i, i + 256, ...), then gdml_md_run's 256-slot tree; v_i . g
 *   and v_i . t: one wavefront per row, lanes stride the columns, the xor butterfly; the back-projection sums over i ascending.
 *   No atomics.  A call makes at most max_steps + 1 evaluations per geometry; E_end, F_end, w_end are always those of R.
 * The driver is gdml_relax_run's general route: plain launches queued back to back, the host synchronises once per chunk
 *   (predict.relax_chunk_steps evaluations, at most predict.md_chunk_frames frames / 64 MiB when R is recorded), reads the
 *   status words and first_bad_step flags and stops when no geometry is active.  When B Hessians and work matrices exceed
 *   gdml_vib_run's 256 MiB, every evaluation walks the geometries in slices (predict.vib_chunk).  No persistent kernel, no
 *   graph, no waiting between workgroups.
 * Arguments.  R (B,3N), trust, E_prev, dE_pred (B), flags (B, int64; bit 0 = a previous step exists, bit 1 = that step was
 *   clipped), t (B,3N) or NULL (the follow vector, e.g. gdml_neb_run's tangent at i_climb; any length): the state, the start on
 *   entry and the end on return.  A fresh start: trust = the first radius, E_prev = dE_pred = 0, flags = 0.  Passing the end
 *   state back continues the run as if it had not been cut (max_steps is the budget of one call).
 *   status (B,2), first_bad_step (B), n_made, record_every, R_rec: exactly as in gdml_relax_run.  E_hist, fmax_hist,
 *   w_follow_hist (max_steps + 1, B): rows 0 .. n_made - 1 are written, E' UNSCALED; a frozen geometry repeats its last value.
 *   k_follow_hist (max_steps + 1, B) int64 or NULL: the same for the followed index.  E_end (B), F_end (B,3N): E', F' UNSCALED
 *   at R.  w_end (B,3N): the spectrum at R in gdml_vib_run's layout (vibrational entries ascending, then n_rigid zeros), with
 *   n_rigid, n_neg (B).  mode_end (B,3N).  The caller checks n_neg == order; the search does not enforce it.
 * Bit-identical: the same call repeated; n steps then a continuation against 2 n steps; any chunk length; any record_every;
 *   steps 2-4 never depend on the batch or the slice, so neither do the results as far as gdml_predict_hessian_dev returns the
 *   same bits for a geometry; w_end is gdml_vib_run's w2 at R with unit masses; E_end, F_end are gdml_predict_hessian_dev's.
 * GDML_ERR_INVALID before any launch (ctx may be NULL for these checks): NULL params, max_steps < 0, record_every < 0 (< 1 with
 *   R_rec), B < 0, N < 1, f_scale <= 0 or not finite, fmax <= 0 or not finite, order outside {0, 1}, trust_min <= 0,
 *   trust_max < trust_min, project outside 0 .. 2, exactly one of lat / lat_inv, project = 2 with a lattice, a follow vector
 *   with order = 0, a NULL state or output array (k_follow_hist, R_rec, t and first_bad_step may be NULL), a trust outside
 *   [trust_min, trust_max], flags outside 0 .. 3, a non-finite E_prev or dE_pred where bit 0 is set, a non-finite coordinate or
 *   follow vector entry; N different from the model's.  GDML_ERR_UNSUPPORTED for N > 197 (the Hessian's limit).  GDML_ERR_STATE
 *   without a model. */
typedef struct gdml_ef_params {
  int64_t B;
  int N;
  int order;             /* 0 minimum, 1 first-order saddle */
  double f_scale;        /* g = -f_scale * F', D = f_scale * H' */
  const double* lat;
  const double* lat_inv; /* both or neither */
  double fmax;           /* converged when the largest |g_atom| is below it */
  double trust_min, trust_max;
  int project;           /* 0 none, 1 translations, 2 translations + rotations */
} gdml_ef_params;        /* 72 bytes */
int gdml_ef_run(gdml_ctx* ctx, const gdml_ef_params* params, double* R, double* trust, double* E_prev, double* dE_pred,
                int64_t* flags, double* t /* or NULL */, int64_t max_steps, int64_t record_every, double* R_rec /* or NULL */,
                double* E_hist, double* fmax_hist, double* w_follow_hist, int64_t* k_follow_hist /* or NULL */, double* E_end,
                double* F_end, double* w_end, int64_t* n_rigid, int64_t* n_neg, double* mode_end, int64_t* status,
                int64_t* first_bad_step);

/* Posterior force covariance of the Gaussian process behind the model (active learning, leaving the training distribution):
 *   cov F(x*) = k(x*,x*) - K*^T (K + lam I)^-1 K*.  The reference has no counterpart (its solve runs on the host and drops the
 * factor).  In the library's conventions -- K the un-negated matrix of gdml_assemble_K, A = -K + lam I = L L^T, labels
 * normalised by std -- and for one query geometry q:
 *   Kx_q (3N x n, n = 3N M): block j = the 3N x 3N block of train.py:97-232 for row point q (un-permuted) and column point j;
 *   k_qq (3N x 3N): the same with i = j = q;   Z_q = (-Kx_q) L^-T;   Sig_q = -k_qq - Z_q Z_q^T.
 * The caller multiplies by std^2.  (The variance of E is not offered: forces fix E up to a constant, its posterior variance
 * stays near 0.7 of the prior everywhere.)
 * gdml_uncert_prepare: needs the training set of gdml_train_upload (Cartesian geometries are not part of a model file: the
 *   caller computes their descriptors, gdml_desc_from_R).  Assembles A (gdml_assemble_A), factors it in place
 *   (gdml_chol_factor: *info > 0 and GDML_ERR_NOT_PD for a matrix that is not positive definite) and marks the factor as
 *   prepared.  The n x n matrix stays resident; anything that overwrites it (an assembly, a Nystroem build, an LU, a new
 *   training set) clears the mark.  gdml_uncert_release frees the matrix and the work buffers.
 * gdml_uncert_cross: host copies of the UN-negated Kx (B 3N x n) and k_qq (B,3N,3N) of B host geometries (either may be
 *   NULL).  Needs only the training set, not the factor; the length scale is that of the last assembly on the context
 *   (gdml_uncert_prepare, gdml_assemble_*), else the uploaded model's.
 * gdml_predict_cov: cov_out (B,3N) marginal variances (full = 0) or (B,3N,3N) covariances (full != 0, both triangles), R
 *   (B,3N) host geometries; the _dev variant takes device pointers for R and the output and gives the same bits.  fp64
 *   throughout (the Gram step on the MFMA pipe), no atomics: repeated calls give bit-identical results and the variances
 *   equal the diagonal of the full form bit for bit.  Batches go through in chunks (option predict.cov_chunk).
 * GDML_ERR_STATE without a prepared factor, GDML_ERR_INVALID for a NULL R, B < 0 or a lattice without its inverse,
 * GDML_ERR_UNSUPPORTED when the resident system carries energy-constraint rows. */
int gdml_uncert_prepare(gdml_ctx* ctx, double sig, double lam, int* info);
int gdml_uncert_release(gdml_ctx* ctx);
int gdml_uncert_cross(gdml_ctx* ctx, const double* R, int64_t B, const double* lat, const double* lat_inv,
                      double* Kx_out, double* kqq_out);
int gdml_predict_cov(gdml_ctx* ctx, const double* R, int64_t B, const double* lat, const double* lat_inv, int full,
                     double* cov_out);
int gdml_predict_cov_dev(gdml_ctx* ctx, const double* R_dev, int64_t B, const double* lat, const double* lat_inv,
                         int full, double* cov_dev);

/* The same covariance for a handful of geometries at low latency (one geometry per step of an MD loop): Sig_q = -k_qq - Z_q Z_q^T,
 * Z_q = (-Kx_q) L^-T as above, with a forward solve made for r = 3N B <= GDML_COV_FEW_ROWS rows (one geometry of up to 85 atoms,
 * two of 42, four of 21): steps of 256 columns, the diagonal part through per-call inverses of the 64 x 64 diagonal blocks of L and
 * MFMA sub-updates, the trailing update in strips that read L exactly once (csrc/uncert_few.hip).  Arguments, units, states and
 * error codes are those of gdml_predict_cov[_dev]; B = 0 is a no-op; the factor and the training set are only read.
 * When 3N B exceeds the limit (option predict.cov_few_rows, default and maximum GDML_COV_FEW_ROWS, 0 = never) the call IS
 * gdml_predict_cov[_dev], with its bits, so callers need not know the limit.  Within the limit the results agree with
 * gdml_predict_cov to rounding (another summation order), not bit for bit.
 * Invariants of the path within the limit:
 *   1. repeated calls give identical bits;
 *   2. the _dev entry equals the host entry bit for bit;
 *   3. the variances (full = 0) equal the diagonal of the full form bit for bit;
 *   4. a geometry's result does not depend on which other geometries share the call, nor on its position in it, bit for bit;
 *   5. gdml_predict_cov, gdml_loo and gdml_chol_solve give the same bits before and after a call;
 *   6. the path works at once on the factor left by gdml_factor_extend / gdml_factor_remove.
 * Not offered: factors with energy-constraint rows (GDML_ERR_UNSUPPORTED) or of a multi-rank context, inverses cached across
 * calls, a persistent single-launch form, bit equality with gdml_predict_cov.  Timers: phase "uncert_few"; kernels "few_cross",
 * "few_inv", "few_solve" (or "few_diag" / "few_upd", see predict.cov_few_split_timers), "few_gram". */
#define GDML_COV_FEW_ROWS 256
int gdml_predict_cov_few(gdml_ctx* ctx, const double* R, int64_t B, const double* lat, const double* lat_inv, int full,
                         double* cov_out);
int gdml_predict_cov_few_dev(gdml_ctx* ctx, const double* R_dev, int64_t B, const double* lat, const double* lat_inv,
                             int full, double* cov_dev);

/* Leave-one-out force errors, their predictive covariances and log det A from the resident Cholesky factor: what M
 * retrainings on M - 1 points each would give, in one pass (Rasmussen & Williams, Gaussian Processes for Machine Learning,
 * 5.4.2, in block form).  The reference has no counterpart (it holds back a validation split).  In the library's conventions --
 * A = -K + lam I = L L^T, labels y normalised by std, alphas = -A^-1 y as gdml_chol_solve returns them -- and with a = -alphas,
 * a_j the 3N entries of training point j and G_j the 3N x 3N diagonal block j of A^-1:
 *   r_j = G_j^-1 a_j = y_j - (prediction at x_j of the model trained without point j)      resid_out (M,3N)
 *   C_j = G_j^-1     = predictive covariance of the left-out label, noise lam included      cov_out
 *   log det A = 2 sum_i log L_ii                                                             *logdet_out
 * The caller multiplies r by std and C by std^2.  cov_mode 0: cov_out is not written (may be NULL); 1: (M,3N) diagonals of C_j;
 * 2: (M,3N,3N), both triangles.  alphas (n = 3N M) are host coefficients that belong to the resident factor's matrix: for
 * coefficients from another solver (PCG to 1e-4) solve y through the factor first (gdml_chol_solve).
 * Needs a factor WITHOUT energy-constraint rows resident for the training set of gdml_train_upload: after gdml_uncert_prepare,
 * or after gdml_chol_factor / gdml_chol_solve in training (the right-hand-side row behind the factor is not touched).  The
 * factor is only read: a prepared factor stays prepared, gdml_predict_cov gives the same bits before and after.
 * fp64 throughout (G_j on the MFMA pipe), no atomics, every sum in a fixed order: repeated calls give identical bits, the
 * diagonal of cov_mode 2 and resid_out equal those of cov_mode 1 bit for bit, and nothing depends on option chol.loo_chunk.
 * GDML_ERR_STATE without a factor or with one that does not belong to the training set, GDML_ERR_UNSUPPORTED for a factor
 * with energy-constraint rows or a multi-rank context, GDML_ERR_INVALID for NULL arguments / a wrong n / cov_mode,
 * GDML_ERR_NOT_PD with *info = j + 1 when G_j of training point j has a non-positive pivot (the outputs are then undefined).
 * Not offered: leave-one-out energies (the integration constant is refitted per fold) and systems with energy constraints. */
int gdml_loo(gdml_ctx* ctx, const double* alphas, int64_t n, int cov_mode, double* resid_out, double* cov_out,
             double* logdet_out, int* info);

/* Gradient of the model evidence (log marginal likelihood) in the length scale sig and the regularisation lam from the resident
 * Cholesky factor: what type-II maximum likelihood needs to set both without a grid and without held-back data.  The reference
 * has no counterpart (it picks an integer sig by validation error and never tunes lam).  In the library's conventions -- K the
 * un-negated kernel matrix, A = -K + lam I = L L^T, labels y normalised by std, a = A^-1 y = -alphas, model y ~ N(0, s^2 A),
 *   lml = -1/2 y^T a / s^2 - 1/2 (log det A + n log s^2) - n/2 log 2 pi                     (GDMLPredict.loo_errors)
 * -- and with K' = dK/dsig at the factor's own sig (the sig of the assembly the factor came from):
 *   d lml / d sig = 1/2 ( <A^-1, K'> - a^T K' a / s^2 ),     <X, Y> = sum_ij X_ij Y_ij
 *   d lml / d lam = 1/2 ( a^T a / s^2 - tr A^-1 )
 * at fixed s^2; at the maximum-likelihood s^2 = y^T a / n these are the total derivatives of the profiled evidence.
 *   terms_out[5] = { tr A^-1, <A^-1, K'>, a^T K' a, a^T a, log det A }
 * The caller combines them with s^2: the library knows nothing of labels or s^2, as gdml_loo knows nothing of them.  K' has the
 * block structure of K: for a pair of points, a permutation p, d = x_i - P_p x_j, r = sqrt(5) |d|, e = exp(-r / sig) the block
 * J_i^T [f1 d d^T - f2 I] J_j^p of K (f1 = 25 e / (3 sig^4), f2 = 5 e (sig + r) / (3 sig^3)) becomes that of K' with
 *   f1' = f1 (r - 4 sig) / sig^2,     f2' = 5 e (r^2 - 2 sig r - 2 sig^2) / (3 sig^5);
 * it is contracted against the tiles of A^-1 on the fly and never assembled or stored.
 * alphas (n = 3N M): host coefficients that belong to the resident factor's matrix (gdml_chol_solve), as for gdml_loo.
 * Three passes, chunk by chunk over the training points (option chol.evidence_chunk): the rows of Z = L^-T by the seed and the
 * right-looking solve of gdml_loo, solved in the chunk buffer and the true rows (not the rows padded to 128 behind them) copied
 * into a SECOND n x pitch matrix that is allocated for the call; the rows of -A^-1 up to the diagonal, one GEMM per chunk; the
 * contraction kernel over the lower block triangle (off-diagonal pairs count twice).  MEMORY: the second matrix is as large
 * as the factor (31.7 GB at n = 63 000), so the call needs twice the factor's memory; GDML_ERR_OOM, with the bytes needed
 * and the bytes free in the message, when it does not fit.
 * Invariants: the factor and the training set are only read -- gdml_predict_cov, gdml_loo and gdml_chol_solve give the same
 * bits before and after a call; every buffer of the call is released on every exit path; fp64 throughout, no atomics, every
 * sum in a fixed order (the four sums stay apart down to the host): repeated calls give identical bits; log det A is
 * gdml_loo's, bit for bit; different values of chol.evidence_chunk agree to rounding, not bit for bit.
 * Needs what gdml_loo needs: a factor WITHOUT energy-constraint rows resident for the training set of gdml_train_upload on a
 * single-rank context.  GDML_ERR_STATE without a factor or with one that does not belong to the training set,
 * GDML_ERR_UNSUPPORTED for a factor with energy-constraint rows or a multi-rank context, GDML_ERR_INVALID for NULL arguments
 * or a wrong n.  *info is set to 0 (optional).  Phase "evidence"; kernel timers evidence_seed, evidence_solve, evidence_inv,
 * evidence_contract.
 * Not offered: energy-constraint systems, multi-GPU factors, gradients of the leave-one-out error, per-atom-type or anisotropic
 * length scales, a stochastic (Hutchinson) trace estimate for systems whose second matrix does not fit. */
int gdml_evidence_grad(gdml_ctx* ctx, const double* alphas, int64_t n, double* terms_out /* 5 */, int* info);

/* Appending b training points to the factor of gdml_uncert_prepare without factoring again (on-the-fly learning: label the
 * geometries gdml_predict_cov flags, add them, go on).  The reference has no counterpart (it retrains from nothing).  With
 * A = -K + lam I = L L^T resident (n = 3N M) and m = 3N b new rows the factor is bordered,
 *   A' = | A  C^T |    L' = | L  0   |    C = -Kx of the new points against the old ones,  W = C L^-T,
 *        | C  D   |         | W  L_S |    S = D - W W^T = L_S L_S^T,
 * at n^2 m flops instead of n'^3 / 3: the cross-kernel rows of gdml_predict_cov, its right-looking triangular solve, a split-k
 * Gram product on the fp64 MFMA pipe and the blocked Cholesky on the m x m Schur complement, in chunks of at most
 * chol.extend_chunk points (a chunk's rows are part of the factor the next chunk solves against).
 * R_desc_new (b,D), R_d_desc_new (b,D,3): host descriptors and compressed Jacobians of the new points (gdml_desc_from_R);
 * they are appended to the resident training set, the new factor (n' = n + m rows, pitch n' rounded up to 16) replaces the
 * old one and stays prepared: gdml_chol_solve, gdml_predict_cov and gdml_loo work on the enlarged system at once; sig and
 * lam are those of gdml_uncert_prepare.  The new rows are built in a second buffer, so both matrices are resident for the
 * duration of the call, and the context changes only after the last chunk has been factored: on ANY error the old factor,
 * the old training set and the prepared mark are exactly as before.  b = 0 is a no-op.
 * fp64 throughout, no atomics, every sum in a fixed order: the same sequence of calls on the same context state gives
 * identical bits (different chunkings of the same points agree to rounding only).
 * GDML_ERR_STATE without a prepared factor of the resident training set, GDML_ERR_UNSUPPORTED for a factor with
 * energy-constraint rows or a multi-rank context, GDML_ERR_INVALID for b < 0 or NULL tables, GDML_ERR_OOM when the second
 * buffer does not fit, GDML_ERR_NOT_PD with *info = order of the failing leading minor of A' (1-based) when a pivot of S is
 * not positive.  Phase "extend"; kernel timers extend_copy, extend_cross, extend_solve, extend_schur, extend_chol.
 * Not offered: systems with energy constraints, a reserved pitch that would avoid the copy (removing points:
 * gdml_factor_remove). */
int gdml_factor_extend(gdml_ctx* ctx, const double* R_desc_new, const double* R_d_desc_new, int64_t b, int* info);

/* Removing b training points from the factor of gdml_uncert_prepare without factoring again (a label that turned out wrong
 * under gdml_loo, a window of fixed size over a trajectory).  The reference has no counterpart.  idx: b distinct host indices
 * of training points in the resident order; the kept points keep their relative order.  With L_c = L[kept, kept] and
 * V = L[kept, removed] (m = 3N b columns)
 *   A_kept = L_c L_c^T + V V^T = L' L'^T,   [L_c V] Q = [L' 0]  with Q orthogonal:
 * a rank-m positive update of the rows behind the first removed point, at O(m n^2) flops and one read and write of the
 * factor instead of n'^3 / 3.  L_c and V are gathered into a second buffer (n' = n - m rows, pitch n' rounded up to 16) and
 * a side buffer; then, 64 columns at a time, a Householder LQ of [L_kk V_k] in one workgroup (reflectors e_i + [0; v_i],
 * kept as a WY pair) and its application to the rows below on the fp64 MFMA pipe.  V goes through in slices of at most
 * chol.remove_chunk points and 128 columns, highest columns first; a slice's sweep leaves the other slices' columns alone.
 * Removing only the LAST points is a truncation: no sweep runs.  A diagonal entry that comes out negative has its column
 * negated (gdml_loo sums logs of positive entries).
 * The resident training set loses the points, the new factor replaces the old one and stays prepared: gdml_chol_solve,
 * gdml_predict_cov, gdml_loo and gdml_factor_extend work on the reduced system at once.  Both matrices are resident for the
 * duration of the call, and the context changes only after the last sweep: on ANY error the old factor, the old training
 * set and the prepared mark are exactly as before.  b = 0 is a no-op.
 * fp64 throughout, no atomics, every sum in a fixed order: the same sequence of calls on the same context state gives
 * identical bits (different values of chol.remove_chunk agree to rounding only).
 * GDML_ERR_STATE without a prepared factor of the resident training set, GDML_ERR_UNSUPPORTED for a factor with
 * energy-constraint rows or a multi-rank context, GDML_ERR_INVALID for b < 0, NULL idx with b > 0, an index outside
 * [0, M), a duplicate or b = M (nothing left), GDML_ERR_OOM when the second buffer does not fit, GDML_ERR_NOT_PD with
 * *info = column of the reduced system (1-based) whose new diagonal entry is not positive and finite.
 * Phase "remove"; kernel timers remove_compact, remove_panel, remove_apply.
 * Not offered: systems with energy constraints, replacing a point in place, a reserved pitch that would avoid the copy. */
int gdml_factor_remove(gdml_ctx* ctx, const int64_t* idx, int64_t b, int* info);

/* Choosing which n_select of B unlabelled candidate geometries to label next, by the greedy batch rule on the JOINT information
 * gain (ranking gdml_predict_cov's variances scores every geometry alone: a pool cut from a trajectory is full of near-copies
 * and the top of that ranking is one geometry several times).  The reference has no counterpart.  With A = -K + lam I = L L^T
 * resident (n = 3N M, n3 = 3N), T the training set, S_t the candidates picked before step t and, for candidate q,
 *   W_q = (-Kx_q) L^-T,   Sig_q^(0) = -k_qq - W_q W_q^T            (the covariance gdml_predict_cov returns, bit for bit)
 *   gain_t(q) = log det(Sig_q^(t) / lam + I) = log det A_{T+S_t+q} - log det A_{T+S_t} - n3 log lam      (nats)
 * -- twice the mutual information between the model and a noisy label at q given everything known so far; it needs no labels
 * and does not depend on std -- step t picks q* = argmax gain_t (ties: the LOWEST pool index) and conditions the pool on it:
 *   C = -k(pool, q*) - W W_q*^T - sum_{s<t} V_s V_s[q*]^T  (n3 B x n3),   V_t = C G^-T  with  G G^T = Sig_q*^(t) + lam I,
 *   Sig_q^(t+1) = Sig_q^(t) - V_t[q] V_t[q]^T   for every remaining q,
 * a block-pivoted Cholesky of the pool's joint posterior covariance.  The sweep ends after n_select picks, or before a pick
 * whose gain is below min_gain (-inf: never).  W W_q*^T runs on the fp64 MFMA pipe and reads all of W ceil(n3 / 64) times per step.
 * R (B,3N) host geometries; gain0_out (B) the initial gains of ALL candidates; idx_out, gain_out (n_select) the picks in
 * order and their gains at the time of the pick, of which *n_selected_out are written.  With n_select = 0 only gain0_out is
 * computed, the candidates stream through in chunks (option chol.select_chunk) and any pool size works; n_select = 1 adds an
 * argmax to that and retains nothing either; otherwise W (n3 B x n),
 * the covariances and the block columns V stay on the device for the duration of the call.
 * The factor and the training set are only read: a prepared factor stays prepared, gdml_predict_cov, gdml_loo and
 * gdml_chol_solve give the same bits before and after.  fp64 throughout, no atomics, every sum in a fixed order: repeated
 * calls give identical bits; a candidate's initial gain depends neither on its place in the pool nor on chol.select_chunk (two
 * identical geometries have identical initial gains), and different values of chol.select_chunk give the same picks.
 * GDML_ERR_STATE without a prepared factor of the resident training set, GDML_ERR_UNSUPPORTED for a factor with
 * energy-constraint rows or a multi-rank context, GDML_ERR_INVALID for a NULL R, B < 0, n_select outside [0, B], a lattice
 * without its inverse, a NULL gain0_out / n_selected_out or (n_select > 0) idx_out / gain_out, GDML_ERR_OOM when the retained
 * buffers do not fit -- the message ends with "largest pool that fits: K" (0: none of at least n_select candidates) --,
 * GDML_ERR_NOT_PD with *info = q + 1 when Sig_q + lam I of candidate q has a non-positive pivot.  After any error every work
 * buffer of the call has been released.  Phase "select"; kernel timers select_cross, select_solve, select_gram, select_score,
 * select_column, select_update.
 * Not offered: systems with energy constraints, multi-GPU factors, criteria other than the information gain, removing
 * candidates from a running sweep, labelling (gdml_factor_extend adds the labelled points). */
int gdml_select_points(gdml_ctx* ctx, const double* R, int64_t B, const double* lat, const double* lat_inv, int64_t n_select,
                       double min_gain, int64_t* idx_out, double* gain_out, double* gain0_out, int64_t* n_selected_out,
                       int* info);

/* Test / validation error sums evaluated on the device (replaces the body of the reference's
 * cli.test loop, sgdml/cli.py:1564-1605 with _online_err :1170): predicts B host geometries R,
 * scales with std and c like predict.py:1286-1288, compares with the labels and returns
 *   sums8_out = { sum|dE|, sum dE^2, sum|dF|, sum dF^2, sum|d|F||, sum(d|F|)^2, sum a, sum a^2 },
 * a = arccos(clip(cos(f_pred, f_ref)))/pi per atom.  E_ref may be NULL (sums 0, 1 are then 0).
 * The caller divides by the sample sizes exactly as _online_err does. */
int gdml_predict_errors(gdml_ctx* ctx, const double* R, int64_t B, const double* lat,
                        const double* lat_inv, double std, double c, const double* E_ref,
                        const double* F_ref, double* sums8_out);

/* Kernel mat-vec  out = K v - lam v  through the prediction contraction (replaces
 * Iterative._K_vec, sgdml/solvers/iterative.py:183-204).  n = 3NM (+M with E constraints). */
int gdml_kernel_matvec(gdml_ctx* ctx, double lam, int use_E_cstr, const double* v, int64_t n,
                       double* out);

/* ---- iterative solver (replaces sgdml/solvers/iterative.py) ------------------------------
 * gdml_nystroem_factor (iterative.py:208-351 + :414-471): requires the (n+m) x m matrix of
 *   gdml_assemble_K(GDML_COLS_INDEX, idx, m, alloc_extra_rows = m).  Computes on the device
 *   L^-1 K_mn (m x n) with the jitter-escalation semantics of _cho_factor_stable, keeps it
 *   resident as the preconditioner, returns the leverage scores (column squared norms,
 *   iterative.py:107-109) in lev_scores_out (n) and optionally the factor in
 *   LinvKmn_host_out (m x n row-major, may be NULL).  *info: bits 8.. = number of jitter escalations the Cholesky of
 *   K_mm needed (iterative.py:442-463); bit 0 = the second Cholesky failed and
 *   the alternative branch ran (the reference's QR of [K_nm; sqrt(lam) I], iterative.py:313-324; here a
 *   shifted CholeskyQR3 on fp64 MFMA with the same R^T R up to rounding).
 *   lev_scores_out may be NULL: the scores are then computed on demand by gdml_nystroem_lev_scores (valid until the next
 *   assembly overwrites the matrix).  *info bit 1 / bit 2: the preconditioner will be applied matrix-free / from the fp32
 *   copy of the factor (option pcg.precon_form); the matrix-free form skips the second tall triangular solve of the factor
 *   until somebody asks for the scores.
 * gdml_precon_apply: out = (L^T L v - v)/lam  (iterative.py:120-140).  Matrix-free form: with X = L^-1 K_mn = Z^T K_mn,
 *   Z = L_mm^-T L^-T (m x m), L^T L v = K_nm Z Z^T K_mn v: K_mn v is gdml_kernel_matvec followed by a gather of the m inducing
 *   entries, K_nm t a scatter followed by the mat-vec; the n x m factor is not read.  fp32 form: (X32 T0 X32^T v - v)/lam.
 * gdml_pcg: preconditioned CG for (-K + lam I) x = y with scipy.sparse.linalg.cg semantics
 *   (iterative.py:740-752: rtol*||y||, atol = 0, x0 optional).  Vectors and CG scalars stay on the device; the host
 *   reads the residual of an iteration only when it queues the iteration `pcg.depth` (default 2) steps later, so the GPU
 *   never waits for the host, and returns exactly the iterate scipy would (the iterates in flight live in a ring).
 *   cb(iter, resid, user) is called every cb_every iterations (0 = never) with resid = ||y - A x_iter|| (the recurrence
 *   residual after the update, what the reference's callback reads from scipy's frame, iterative.py:626-632); a non-zero
 *   return stops the solve with x_iter (used for CGRestartException, iterative.py:729).  Inside the callback -- and only
 *   there -- gdml_pcg_x copies x_iter to the host (checkpoints, iterative.py:675-735; restarts): the iterate does not
 *   cross PCIe unless somebody asks for it.
 *   info_out: 0 converged, 1 maxiter reached, 2 stopped by callback. */
typedef int (*gdml_pcg_cb)(int64_t iter, double resid, void* user);
int gdml_nystroem_factor(gdml_ctx* ctx, double lam, const int64_t* idx, int64_t m,
                         double* lev_scores_out, double* LinvKmn_host_out, int* info);
int gdml_nystroem_lev_scores(gdml_ctx* ctx, double* lev_scores_out);
int gdml_precon_apply(gdml_ctx* ctx, double lam, const double* v, int64_t n, double* out);
int gdml_pcg(gdml_ctx* ctx, double lam, int use_E_cstr, const double* y, const double* x0,
             int64_t n, double rtol, int64_t maxiter, int use_precon, gdml_pcg_cb cb,
             int64_t cb_every, void* user, double* x_out, int64_t* iters_out, double* resid_out,
             int* info_out);
int gdml_pcg_x(gdml_ctx* ctx, double* x_host_out);

/* ---- multi-GPU (new: the reference has no collective) ----------------------
 * One process per GPU.  Rank 0 calls gdml_comm_unique_id (128 bytes) and ships it to the
 * other ranks by any host channel (sgdml_amd/dist.py uses torch.distributed's store); every rank then
 * calls gdml_comm_init (id128 = NULL: "virtual rank" without a communicator, shard arithmetic only --
 * tests).  After that
 *   - the iterative path is sharded over the training points (contiguous row shards):
 *     gdml_assemble_K(GDML_COLS_INDEX, ..., alloc_extra_rows > 0) assembles the rank's rows of K_nm,
 *     gdml_nystroem_factor / gdml_precon_apply / gdml_kernel_matvec / gdml_pcg exchange m- and n-vectors with
 *     RCCL all-reduce / all-gather over xGMI; with use_E_cstr a rank holds the force rows of its points followed by their
 *     energy rows (vectors cross the ABI in the reference order -- forces, then energies -- on every rank; the rank-major
 *     order of the device vectors stays inside the library);
 *   - the analytic path is gdml_dist_chol_solve (block-row-cyclic matrix, below).
 * The collectives are issued for every communicator size, including one rank.  gdml_chol_* / gdml_lu_solve stay
 * single-GPU entry points. */
int gdml_comm_unique_id(void* id128_out);
int gdml_comm_init(gdml_ctx* ctx, const void* id128, int rank, int world);
int gdml_comm_info(gdml_ctx* ctx, int* rank_out, int* world_out);
/* gdml_comm_suspend(ctx, 1) parks the communicator: until gdml_comm_suspend(ctx, 0) the context behaves like a single GPU
 * without one (rank 0 of 1: unsharded assembly, local Cholesky / LU / PCG, no collective).  For work every rank performs
 * redundantly on its own GPU because the sharded solvers do not carry it: the LU branch of a matrix that is not positive
 * definite (analytic.py:101-114).  (Energy constraints, train.py:235-300, are carried by both sharded solvers since round 6.) */
int gdml_comm_suspend(gdml_ctx* ctx, int suspend);

/* Distributed analytic solve (new; Analytic.solve, analytic.py:65-99, for systems beyond one GPU -- BASELINE.json
 * configs[3], [4]): the system matrix A = -K + lam I is assembled block-ROW-cyclic over the ranks of the communicator
 * (512-row blocks, every rank only its own rows: n^2 * 8 / world bytes per GPU), factored by a right-looking blocked
 * Cholesky (diagonal block broadcast, row-local panel solve, panel all-gather over RCCL, local fp64-MFMA trailing
 * update) with the right-hand side carried as a replicated extra row, and solved back; every rank receives
 * alphas = -(A^-1 y).  n = 3N M, or 3N M + M for a system with energy constraints (train.py:235-300: y then carries the M
 * energy labels behind the forces, the energy rows are assembled on the ranks that own them).  Needs gdml_train_upload (any P)
 * and a communicator (gdml_comm_init / gdml_comm_init_host; without one it runs on a single GPU).  *info as gdml_chol_factor. */
int gdml_dist_chol_solve(gdml_ctx* ctx, double sig, double lam, const double* y, int64_t n, double* alphas_out,
                         int* info);

/* Host-staged collectives: the same sharded algorithms with the two collectives delegated to the caller
 * (e.g. torch.distributed's gloo backend).  The library copies the device buffer to pinned host memory,
 * calls the callback, which must complete the collective IN PLACE on that host buffer, and copies it back.
 *   allreduce(buf, count, user): buf[0:count] <- sum over ranks
 *   allgather(buf, chunk, user): buf holds world*chunk doubles, rank r's contribution at [r*chunk, (r+1)*chunk)
 * A non-zero return aborts the calling operation with GDML_ERR_COMM.  Used where RCCL cannot run: several
 * ranks sharing one GPU (tests of the sharded code path on a one-GPU box), or a node without xGMI peers. */
typedef int (*gdml_host_allreduce)(double* buf, int64_t count, void* user);
typedef int (*gdml_host_allgather)(double* buf, int64_t chunk, void* user);
int gdml_comm_init_host(gdml_ctx* ctx, int rank, int world, gdml_host_allreduce allreduce,
                        gdml_host_allgather allgather, void* user);

/* Collectives issued and payload bytes handed to them by this rank since the communicator was set up. */
int gdml_comm_stats(gdml_ctx* ctx, int64_t* calls_out, double* bytes_out);

/* ---- raw device buffers for callers that keep data resident -------------------------- */
int gdml_dev_alloc(gdml_ctx* ctx, int64_t bytes, void** dev_out);
int gdml_dev_free(gdml_ctx* ctx, void* dev);
int gdml_memcpy_h2d(gdml_ctx* ctx, void* dev, const void* host, int64_t bytes);
int gdml_memcpy_d2h(gdml_ctx* ctx, void* host, const void* dev, int64_t bytes);

/* Device pointer + leading dimension of the resident kernel matrix / factor (for tests). */
int gdml_K_dev(gdml_ctx* ctx, double** K_dev_out, int64_t* ld_out);

#ifdef __cplusplus
}
#endif
#endif /* GDML_HIP_H */

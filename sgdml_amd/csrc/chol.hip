// Analytic solve on gfx950: blocked fp64 Cholesky on the MFMA pipe + triangular solves.
//
// Replaces scipy.linalg.cho_factor / cho_solve as called by Analytic.solve
// (sgdml/solvers/analytic.py:94-99; LAPACK dpotrf/dpotrs underneath) and the Cholesky / TRSM /
// SYRK steps of Iterative._nystroem_cholesky_factor (sgdml/solvers/iterative.py:263-345).
//
// Storage: row-major, LOWER triangle referenced (A = L L^T, L overwrites the lower triangle; the
// strict upper triangle is scratch and may be overwritten with garbage).
//
// Right-looking blocked algorithm, panel width NB (512), ONE stream.  Per panel k:
//   gemm_nt_sub            columns of panel k+1:  C[t0:n, t0:t1] -= P P^T                     (K = NB)
//   gemm_nt_sub_diag       the rest of the trailing matrix (SYRK, lower tiles); workgroup 0 of this launch factors
//                          the NB x NB diagonal block of panel k+1 meanwhile (diag_block_role: potrf64_wg, substitution,
//                          MFMA rank-64 updates) -- the dependent step chain is hidden inside the big launch
//   panel_trsm             row-local solve of the rows below that block, one launch (strip in registers, MFMA updates)
// Near the end (SYRK shorter than the single-workgroup block factorisation) and for the first / ragged panels the
// block is factored by the multi-workgroup 64-wide step chain (potrf_trsm64 + K = 64 GEMM) instead.
// A right-hand side stored as an extra row is carried through (forward substitution for free); the backward
// substitution is one persistent launch with a per-block fallback.  n^3/3 of the flops are in gemm_nt_sub.
// The round-1 schedule (step chain on a second stream with one panel of look-ahead; profiles/r02_panel_fusion_ab.txt), the
// CU-masked / split-stream / chunked variants of rounds 1-2 (profiles/r01_chol_timeline_split.txt, r02_sched_probe.txt) and the
// two-level, persistent and narrow-tile forms of round 6 were measured slower and are gone.
// While the trailing matrix is large (chol.deep, chol.deep_min_rows) the tiles right of the current block of 4096 columns do
// not take part in every outer step: they receive the block in one pass of depth 4096 that rides, as further segments, in the
// launches of the next block's outer steps (gemm_nt_sub_seg_kernel).
//
// Host side, one path: plan -> launch description -> launcher.  chol_plan_build (tile_sched.h, host only: the CPU tests walk
// what runs) clamps the options and lists the operations, every fused launch with its full description (PlanLowerLaunch
// one-level, PlanSegLaunch composed) and the tile counter's target; launch_gemm_lower / launch_gemm_seg turn a description
// into kernel arguments; chol_factor_device runs the list, one call per operation.  The public launch_gemm_nt_sub / _neg /
// _cyclic share launch_gemm_plain.  The triangular solves and the C entries are in chol_solve.hip.
#include "common.h"
#include "tile_sched.h"
#include <array>
#include <memory>
#include <type_traits>
#include <utility>

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------
// C[M x N] -= A[M x K] * B[N x K]^T     (row-major, leading dimensions lda/ldb/ldc)
// lower != 0: C is square-symmetric-updated, only tiles with tile_row >= tile_col are computed.
// Workgroup: 256 threads = 4 waves (2 x 2), tile 128 x 128, each wave 64 x 64 = 4 x 4 MFMA tiles.
// LDS: two stages of the A and B tiles in the 16-byte layout of gemm_store_tile16.  The array keeps the pitch-17 size
// (GT * GPITCH doubles per operand and stage) of the round-1 8-byte layout: the diagonal-block role of the fused launch
// uses it as its scratch.
// ------------------------------------------------------------------------------------------
#define GT 128
#define GBK 16
#define GPITCH 17

struct GemmArgs {
  const double* A;
  const double* B;
  double* C;
  int64_t M, N, K, lda, ldb, ldc;
  int lower;
  int tiles_m, tiles_n;
  int64_t n_super;  // number of 8x8 super tiles enumerated
  int64_t s_begin;  // first super tile of this launch (a launch may cover a sub-range)
  int super_n;      // super-tile columns
  int aligned;      // A, B 16-byte aligned with even leading dimensions (vector loads legal)
  // block-row-cyclic lower structure (distributed Cholesky): C rows are LOCAL rows, local row block lb (cyc_nb rows)
  // is global block (cyc_lb0 + lb) * cyc_W + cyc_rank; a tile is computed iff its first column (cyc_col0 + col0,
  // global) is not right of its last global row; local rows >= cyc_block_rows (carried right-hand side) take all
  int cyc_W, cyc_rank;
  int64_t cyc_lb0, cyc_nb, cyc_col0, cyc_block_rows;
  // fused launch (gemm_nt_sub_diag_kernel): workgroup 0 factors the next panel's diagonal block meanwhile
  double* diagA;    // top-left element of that nb x nb block (leading dimension ldc), or null
  int diag_nbw;     // nb / 64
  int64_t diag_off; // global index of its first row (LAPACK info)
  int* diag_info;
  // merged trailing update (lower): the first super-tile COLUMN (the next outer panel's own columns) is enumerated
  // first; the tiles of its leading ready_rows x ready_rows tile block (the diagonal block workgroup 0 is about to
  // factor) count themselves into *ready when their C tile is stored, workgroup 0 waits for ready_target
  int col0_first;
  int* ready;
  int ready_target, ready_rows;
  // second, plain (non-symmetric) problem carried by the first tiles2 workgroups of the launch:  C2 -= A2 B2^T,
  // M2 x N2, depth K2, same leading dimensions (the K = NB update of panel b's columns by panel a); tiles above the
  // diagonal of its leading N2 x N2 block are skipped; with `ready` set ITS leading tiles are the counted ones
  const double* A2;
  const double* B2;
  double* C2;
  int64_t M2, N2, K2;
  int tiles2;
  int second_compact;  // its tiles2 workgroups all hold a tile (tile_decode_second)
  // balanced tile list of a lower launch (tile_sched.h, option gemm.balance); 0: the super-tile enumeration
  int bal;
  TileLaunch tl;
};

__global__ void __launch_bounds__(256, 2) gemm_nt_sub_diag_kernel(GemmArgs g);

template <bool FULL>
__device__ __forceinline__ void gemm_load_tile(const double* __restrict__ G, int64_t ld,
                                               int64_t row0, int64_t nrows, int64_t k0, int64_t K,
                                               int tid, d2 (&r)[4]) {
  // 128 rows x 16 k = 1024 chunks of 2 doubles; thread t -> chunks t, t+256, ...: row = c/8, kc = c%8
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    int cidx = tid + 256 * s;
    int row = cidx >> 3, kc = (cidx & 7) * 2;
    int64_t gr = row0 + row, gk = k0 + kc;
    if (FULL) {
      r[s] = *reinterpret_cast<const d2*>(G + gr * ld + gk);
    } else {
      // branch-free guarded load: clamp the address, then zero what is out of range
      int64_t cr = gr < nrows ? gr : nrows - 1;
      int64_t ck0 = gk < K ? gk : K - 1, ck1 = gk + 1 < K ? gk + 1 : K - 1;
      double v0 = G[cr * ld + ck0], v1 = G[cr * ld + ck1];
      d2 v;
      v.x = (gr < nrows && gk < K) ? v0 : 0.0;
      v.y = (gr < nrows && gk + 1 < K) ? v1 : 0.0;
      r[s] = v;
    }
  }
}

// 16-byte layout: element (row, kq = k / 2) is the pair (k, k + 1) of a row, stored at d2 index kq * 128 + (row ^ kq).  One
// ds_write_b128 per chunk instead of two ds_write_b64, one ds_read_b128 per operand block and PAIR of k-steps instead of two
// 8-byte reads; the XOR keeps both conflict free: a group of 8 store lanes holds one row and kq = 0..7 (8 different bank
// quads), a 16-lane read group holds 16 different (row ^ kq) & 15 (searched by script).  The MFMA's k index is
// a label: lane group g = lane >> 4 feeds k = 4 g + s into k-step s (both operands), so that a lane's four k of a tile are
// contiguous.
// Full tiles, 16-byte aligned: wave-uniform base (tile corner + k offset: SGPRs) + the thread's constant 32-bit byte offsets
// (row * ld + kc of its four chunks; a tile spans < 2^31 bytes): saddr-form loads, no 64-bit address arithmetic per k-tile.
// Round 6 measured the same loads as BUFFER loads (tile corner in a resource, lane offset as voffset, k offset as soffset: no
// 64-bit lane arithmetic at all): 2.0-2.2 % SLOWER factorisation on two boxes (profiles/r06_gemm_variants.txt); and issuing
// them 16 MFMAs later (after the first MFMA group): +5.8 % -- the 48 MFMAs between issue and LDS commit are needed.
__device__ __forceinline__ void gemm_load_tile_g(const double* __restrict__ base, const unsigned (&off)[4], d2 (&r)[4]) {
  typedef const __attribute__((address_space(1))) char* gcptr;
  typedef const __attribute__((address_space(1))) d2* gd2ptr;
  const uint64_t p = reinterpret_cast<uint64_t>(base);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p), hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
  gcptr b = (gcptr)(((uint64_t)hi << 32) | lo);
#pragma unroll
  for (int s = 0; s < 4; ++s) r[s] = *(gd2ptr)(b + off[s]);
}

__device__ __forceinline__ void gemm_store_tile16(double* __restrict__ S, int tid, const d2 (&r)[4]) {
  d2* S2 = reinterpret_cast<d2*>(S);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int cidx = tid + 256 * s;
    const int row = cidx >> 3, kq = cidx & 7;
    S2[kq * 128 + (row ^ kq)] = r[s];
  }
}

// OW: overwrite, C = -A B^T (C is not read: the caller need not clear it)
template <bool FULL, bool OW>
__device__ __forceinline__ void gemm_tile_body(const GemmArgs& g, double (*lds)[2][GT * GPITCH], int64_t row0, int64_t col0) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 15, lk = lane >> 4;

  // C -= A B^T as acc = -C; acc += A B^T; C = -acc for interior tiles: the 64 C loads per lane are issued with the first
  // operand tiles (their latency is paid once, together with the prologue's), the epilogue is stores only -- instead of
  // four load->store round trips after the last MFMA.  The sign lives in the accumulator: no negation of A operands in the
  // loop.  f64 MFMA C/D layout: col = lane & 15, row = (lane >> 4) + 4 r.
  // wave-uniform tile corner + 32-bit lane offset: the 64 row addresses stay in SGPRs (saddr form), no address VGPRs
  const int wu = __builtin_amdgcn_readfirstlane(wave);
  double* const Ct = g.C + (row0 + (wu >> 1) * 64) * g.ldc + col0 + (wu & 1) * 64;
  const unsigned coff = (unsigned)lk * (unsigned)g.ldc + (unsigned)li;
  d4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (FULL && !OW) {
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] = -(Ct + (int64_t)(i * 16 + 4 * r) * g.ldc)[coff + j * 16];
      } else {
        acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
      }
    }

  // (a staggered k start per tile, after Tensile's StaggerU, was tried and cost 1.5 %: profiles/r03_gemm_ntc_stagger_ab.txt)
  const int nk32 = (int)((g.K + GBK - 1) / GBK);
  d2 ra[4], rb[4];
  gemm_load_tile<FULL>(g.A, g.lda, row0, g.M, 0, g.K, tid, ra);
  gemm_load_tile<FULL>(g.B, g.ldb, col0, g.N, 0, g.K, tid, rb);
  gemm_store_tile16(lds[0][0], tid, ra);
  gemm_store_tile16(lds[0][1], tid, rb);
  __syncthreads();

  // ---- per k-tile two batches of 8 ds_read_b128 + 32 MFMAs
  const int c16 = lane & 15, gq = lane >> 4;
  // full tiles: saddr-form loads (wave-uniform tile corner + the thread's four constant 32-bit byte offsets)
  unsigned offA[4], offB[4];
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4) {
    const int cidx = tid + 256 * s4;
    offA[s4] = (unsigned)(((int64_t)(cidx >> 3) * g.lda + (cidx & 7) * 2) * 8);
    offB[s4] = (unsigned)(((int64_t)(cidx >> 3) * g.ldb + (cidx & 7) * 2) * 8);
  }
  const double* const Abase = g.A + row0 * g.lda;
  const double* const Bbase = g.B + col0 * g.ldb;
  auto load_ab = [&](int64_t kt_, d2 (&ra_)[4], d2 (&rb_)[4]) {
    if constexpr (FULL) {
      const int64_t ko = kt_ * GBK;
      gemm_load_tile_g(Abase + ko, offA, ra_);
      gemm_load_tile_g(Bbase + ko, offB, rb_);
    } else {
      gemm_load_tile<FULL>(g.A, g.lda, row0, g.M, kt_ * GBK, g.K, tid, ra_);
      gemm_load_tile<FULL>(g.B, g.ldb, col0, g.N, kt_ * GBK, g.K, tid, rb_);
    }
  };
  // read-ahead: the operand pairs of the NEXT half are requested while 16 MFMAs of the current one are still to issue, across
  // the tile boundary (the barrier sits before the tile's last 16 MFMAs)
  auto read_half = [&](d2 (&a_)[4], d2 (&b_)[4], int buf, int h) {
    const int kq = 2 * gq + h;
    const int cx = c16 ^ kq;
    const d2* Ap = reinterpret_cast<const d2*>(lds[buf][0]) + kq * 128 + wm * 64 + cx;
    const d2* Bp = reinterpret_cast<const d2*>(lds[buf][1]) + kq * 128 + wn * 64 + cx;
#pragma unroll
    for (int i = 0; i < 4; ++i) a_[i] = Ap[16 * i];
#pragma unroll
    for (int j = 0; j < 4; ++j) b_[j] = Bp[16 * j];
  };
  auto mfma16 = [&](const d2 (&a_)[4], const d2 (&b_)[4], int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(t ? a_[i].y : a_[i].x, t ? b_[j].y : b_[j].x, acc[i][j], 0, 0, 0);
  };
  d2 a0[4], b0[4], a1[4], b1[4];
  read_half(a0, b0, 0, 0);
  // The last k-tile is peeled -- no conditionals inside the loop, -0.3 % of the factorisation (1322 -> 1318 and 1289 -> 1286 ms
  // on two boxes, profiles/r04_gemm_peel_stagger_ab.txt).  The schedule is pinned by a sched_barrier at EVERY phase boundary:
  // with one missing (between the first MFMA group and the read-ahead) a later, unrelated edit of this file made the scheduler
  // sink the reads behind two groups and the kernel lost 3 % (1322 vs 1282 ms on one box) without any change to this loop's
  // source.  Committing the prefetched tile to LDS 16 MFMAs earlier (so that its ds_writes have drained at the barrier) was
  // measured with it: +0.3 %, not kept.
  auto step = [&](int kt, auto has_next_t) {
    constexpr bool HN = decltype(has_next_t)::value;
    const int cur = kt & 1;
    // (sched_barrier: without the loop's conditionals the machine scheduler hoists the commit and the barrier to the
    //  20th MFMA and sinks the read-ahead behind the last one)
    if constexpr (HN) load_ab(kt + 1, ra, rb);
    __builtin_amdgcn_sched_barrier(0);
    mfma16(a0, b0, 0);
    __builtin_amdgcn_sched_barrier(0);  // (between the groups too: in one region the reads were sunk behind BOTH groups and
    read_half(a1, b1, cur, 1);          //  the third group waited for them -- +3 % factorisation time on a fast box)
    __builtin_amdgcn_sched_barrier(0);
    mfma16(a0, b0, 1);
    __builtin_amdgcn_sched_barrier(0);
    mfma16(a1, b1, 0);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (HN) {
      gemm_store_tile16(lds[cur ^ 1][0], tid, ra);
      gemm_store_tile16(lds[cur ^ 1][1], tid, rb);
      __syncthreads();
      read_half(a0, b0, cur ^ 1, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    mfma16(a1, b1, 1);
    __builtin_amdgcn_sched_barrier(0);
  };
  for (int kt = 0; kt + 1 < nk32; ++kt) step(kt, std::true_type{});
  step(nk32 - 1, std::false_type{});

  // ---- epilogue.  f64 MFMA C/D layout: col = lane & 15, row = (lane >> 4) + 4 r.
  if (FULL) {
    // recompute the store addresses from laundered copies: the compiler otherwise keeps the prologue's 32 load addresses
    // alive across the main loop (spilled to scratch)
    double* Ct2g = Ct;
    unsigned coff2 = coff;
    asm volatile("" : "+v"(Ct2g), "+v"(coff2));
    // (the laundered pointer is generic: back to the global address space, or the 64 stores are FLAT stores)
    __attribute__((address_space(1))) double* Ct2 = (__attribute__((address_space(1))) double*)Ct2g;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) (Ct2 + (int64_t)(i * 16 + 4 * r) * g.ldc)[coff2 + j * 16] = -acc[i][j][r];
    return;
  }
  if constexpr (OW) {  // edge tile of an overwriting product: guarded stores, nothing read
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t gc = col0 + wn * 64 + j * 16 + li;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t gr = row0 + wm * 64 + i * 16 + lk + 4 * r;
          if (gc < g.N && gr < g.M) g.C[gr * g.ldc + gc] = -acc[i][j][r];
        }
    }
    return;
  }
  // edge tile: the accumulator holds A B^T; all loads of a 64x16 column strip are issued before the first use
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double cv[4][4];
    const int64_t gc = col0 + wn * 64 + j * 16 + li;
    const bool cok = gc < g.N;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t gr = row0 + wm * 64 + i * 16 + lk + 4 * r;
        const int64_t cr = gr < g.M ? gr : g.M - 1, cc = cok ? gc : g.N - 1;
        cv[i][r] = g.C[cr * g.ldc + cc];
      }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t gr = row0 + wm * 64 + i * 16 + lk + 4 * r;
        if (cok && gr < g.M) g.C[gr * g.ldc + gc] = cv[i][r] - acc[i][j][r];
      }
  }
}

// block index -> tile (tile_sched.h: XCD-aware 8x8 super tiles, block b runs on XCD b % 8) and the tile's GEMM
template <bool OW>
__device__ __forceinline__ void gemm_block(const GemmArgs& g, double (*lds)[2][GT * GPITCH], int64_t b) {
  if (b < g.tiles2) {  // second problem (workgroup-uniform branch)
    const int tn2 = (int)((g.N2 + GT - 1) / GT);
    int64_t ti, tj;
    if (g.second_compact) {
      tile_decode_second(b, tn2, &ti, &tj);
    } else {
      ti = b / tn2; tj = b - ti * tn2;
      if (ti < tn2 && tj > ti) return;
    }
    GemmArgs h = g;
    h.A = g.A2; h.B = g.B2; h.C = g.C2; h.M = g.M2; h.N = g.N2; h.K = g.K2;
    h.aligned = ((reinterpret_cast<uintptr_t>(g.A2) | reinterpret_cast<uintptr_t>(g.B2)) & 15) == 0 && g.aligned;
    const int64_t row0 = ti * GT, col0 = tj * GT;
    const bool full = (row0 + GT <= h.M) && (col0 + GT <= h.N) && ((h.K & (GBK - 1)) == 0) && h.aligned;
    if (full)
      gemm_tile_body<true, false>(h, lds, row0, col0);
    else
      gemm_tile_body<false, false>(h, lds, row0, col0);
    if (g.ready && ti < g.ready_rows && tj < g.ready_rows) {
      __threadfence();
      __syncthreads();
      if (threadIdx.x == 0) atomicAdd(g.ready, 1);
    }
    return;
  }
  b -= g.tiles2;
  int64_t ti, tj;
  if (g.bal) {
    if (!tile_decode_bal(g.tl, b, &ti, &tj)) return;
  } else if (!tile_decode_super(b, g.lower, g.col0_first, g.tiles_m, g.tiles_n, g.super_n, g.s_begin, g.n_super, &ti, &tj)) {
    return;
  }
  const int64_t row0 = ti * GT, col0 = tj * GT;
  if (g.cyc_W > 0 && row0 + GT <= g.cyc_block_rows) {  // tiles that reach into the carried rhs row take all columns
    const int64_t gb = (g.cyc_lb0 + row0 / g.cyc_nb) * g.cyc_W + g.cyc_rank;  // (tiles never straddle blocks: nb % GT == 0)
    const int64_t grow_last = gb * g.cyc_nb + (row0 + GT - 1) % g.cyc_nb;
    if (g.cyc_col0 + col0 > grow_last) return;
  }
  const bool full = (row0 + GT <= g.M) && (col0 + GT <= g.N) && ((g.K & (GBK - 1)) == 0) && g.aligned;
  if (full)
    gemm_tile_body<true, OW>(g, lds, row0, col0);
  else
    gemm_tile_body<false, OW>(g, lds, row0, col0);
  if (g.ready && g.tiles2 == 0 && ti < g.ready_rows && tj < g.ready_rows) {  // publish the tile (release: every thread's stores, then one count)
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(g.ready, 1);
  }
}

__global__ void __launch_bounds__(256, 2) gemm_nt_sub_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) double lds[2][2][GT * GPITCH];
  gemm_block<false>(g, lds, blockIdx.x);
}


// C = -A B^T: the production loop with the accumulators starting at zero and the epilogue's stores only -- for callers whose C
// is a fresh work buffer (the prediction contractions cleared 1.8 GB per mat-vec at configs[3] only to have it read back)
__global__ void __launch_bounds__(256, 2) gemm_nt_neg_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) double lds[2][2][GT * GPITCH];
  gemm_block<true>(g, lds, blockIdx.x);
}

// ---- balanced tile lists (tile_sched.h), cached per context --------------------------------------------------------
// One entry per (tiles_m, tiles_n, first-column-first, launches, second problem): built on first use, its tables uploaded
// once into one device block; a sigma sweep or repeated training at one size builds nothing and copies nothing.
struct TileSchedEntry {
  TileSched S;
  const uint32_t* dev[2] = {nullptr, nullptr};
};
struct CholPlanEntry;
struct TileSchedCache {
  std::map<std::array<int64_t, 7>, TileSchedEntry> entries;
  std::vector<std::pair<std::array<int64_t, 8>, std::shared_ptr<CholPlanEntry>>> plans;  // plans with composed launches
  char* block = nullptr;
  size_t cap = 0, used = 0;
};

void tile_sched_cache_free(gdml_ctx* ctx) {
  if (!ctx->tile_sched) return;
  if (ctx->tile_sched->block) hipFree(ctx->tile_sched->block);
  delete ctx->tile_sched;
  ctx->tile_sched = nullptr;
}

// the balanced list of a lower launch (tile_sched.h: plan_lower_key names it, plan_lower_sched builds it);
// *out = null: no balanced form for this shape (the caller keeps the super-tile enumeration)
static int tile_sched_get(gdml_ctx* ctx, hipStream_t st, const PlanLowerLaunch& L, const TileSchedEntry** out) {
  *out = nullptr;
  if (!ctx->tile_sched) ctx->tile_sched = new TileSchedCache();
  TileSchedCache* c = ctx->tile_sched;
  const std::array<int64_t, 7> key = plan_lower_key(L);
  auto it = c->entries.find(key);
  if (it == c->entries.end()) {
    TileSchedEntry e;
    plan_lower_sched(L, &e.S);
    if (e.S.ok) {
      const size_t b0 = (e.S.table[0].size() * 4 + 255) & ~(size_t)255, b1 = (e.S.table[1].size() * 4 + 255) & ~(size_t)255;
      const size_t block_bytes = (size_t)8 << 20;
      if (!c->block) {
        HIP_CHECK(ctx, hipMalloc((void**)&c->block, block_bytes));
        c->cap = block_bytes;
      }
      if (b0 + b1 > c->cap) {
        e.S.ok = false;
      } else {
        if (c->used + b0 + b1 > c->cap) {  // full: nothing in flight may still read the old tables
          HIP_CHECK(ctx, hipDeviceSynchronize());
          c->entries.clear();
          c->used = 0;
        }
        char* d = c->block + c->used;
        c->used += b0 + b1;
        if (!e.S.table[0].empty()) HIP_CHECK(ctx, hipMemcpyAsync(d, e.S.table[0].data(), e.S.table[0].size() * 4, hipMemcpyHostToDevice, st));
        if (!e.S.table[1].empty()) HIP_CHECK(ctx, hipMemcpyAsync(d + b0, e.S.table[1].data(), e.S.table[1].size() * 4, hipMemcpyHostToDevice, st));
        HIP_CHECK(ctx, hipStreamSynchronize(st));  // once per entry: any stream may use it from here on
        e.dev[0] = reinterpret_cast<const uint32_t*>(d);
        e.dev[1] = reinterpret_cast<const uint32_t*>(d + b0);
      }
    }
    it = c->entries.emplace(key, std::move(e)).first;
  }
  if (it->second.S.ok) *out = &it->second;
  return GDML_OK;
}

// ---- host side of the GEMM launches: launch_gemm_plain (the public wrappers) and launch_gemm_lower (the plan's fused
// launches).  A lower update takes its tiles from the balanced list of its description where gemm.balance (default 1)
// allows and the shape has one, from the super-tile enumeration otherwise.
// the shape part of the kernel argument; the tile range is the whole super-tile enumeration
static GemmArgs gemm_args(const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, int64_t M, int64_t N,
                          int64_t K, int lower) {
  GemmArgs g = {};
  g.A = A; g.B = B; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.lower = lower;
  g.aligned = ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15) == 0 && (lda % 2 == 0) && (ldb % 2 == 0);
  g.tiles_m = (int)((M + GT - 1) / GT); g.tiles_n = (int)((N + GT - 1) / GT);
  const int64_t sm = (g.tiles_m + 7) / 8, sn = (g.tiles_n + 7) / 8;
  g.super_n = (int)sn;
  g.n_super = lower ? sm * (sm + 1) / 2 : sm * sn;
  return g;
}

// launch `launch` of the balanced list te takes the place of the super-tile range; returns its grid
static int64_t gemm_use_list(GemmArgs* g, const TileSchedEntry* te, int launch) {
  g->bal = 1;
  g->tl = te->S.L[launch];
  g->tl.table = te->dev[launch];
  g->s_begin = g->n_super = 0;
  return te->S.blocks[launch];
}

// grid workgroups of kern under the per-kernel timer `name` (only launches on the timing stream are timed)
static int gemm_issue(gdml_ctx* ctx, hipStream_t st, void (*kern)(GemmArgs), int64_t grid, const GemmArgs& g, const char* name,
                      double flops) {
  const int slot = (st == (ctx->kt_stream ? ctx->kt_stream : ctx->stream)) ? ktime_begin(ctx) : -1;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), 0, st, g);
  ktime_end(ctx, slot, name, flops);
  ctx->launch_counter++;
  HIP_CHECK(ctx, hipGetLastError());
  return GDML_OK;
}

// cyc: block-row-cyclic lower structure (GemmArgs::cyc_W ...); overwrite: C = -A B^T, C not read
static int launch_gemm_plain(gdml_ctx* ctx, hipStream_t st, const double* A, int64_t lda, const double* B, int64_t ldb, double* C,
                             int64_t ldc, int64_t M, int64_t N, int64_t K, int lower, const CyclicLower* cyc, bool overwrite) {
  if (M <= 0 || N <= 0 || K <= 0) return GDML_OK;
  GemmArgs g = gemm_args(A, lda, B, ldb, C, ldc, M, N, K, lower);
  if (cyc) { g.cyc_W = cyc->W; g.cyc_rank = cyc->rank; g.cyc_lb0 = cyc->lb0; g.cyc_nb = cyc->nb; g.cyc_col0 = cyc->col0; g.cyc_block_rows = cyc->block_rows; }
  const TileSchedEntry* te = nullptr;
  if (lower && !cyc && !overwrite && ctx_opt(ctx, "gemm.balance", 1) != 0) GDML_TRY(tile_sched_get(ctx, st, plan_lower_plain(M, N, K), &te));
  const int64_t blocks = te ? gemm_use_list(&g, te, 0) : (g.n_super + 7) / 8 * 512;  // each group of 8 super tiles = 8 XCDs x 64 blocks
  if (blocks == 0) return GDML_OK;
  const double flops = lower ? (double)M * (double)(M + 1) * (double)K : 2.0 * (double)M * (double)N * (double)K;  // algorithmic
  return gemm_issue(ctx, st, overwrite ? gemm_nt_neg_kernel : gemm_nt_sub_kernel, blocks, g, "gemm_nt_sub", flops);
}

// Fused launch of the factorisation: the lower update L.upd of the matrix A (leading dimension ld; one launch of its tile
// list), in front of it the second problem where this launch carries it, and as workgroup 0 the diagonal block at L.diag0,
// which waits for ready_target counted tiles where L.counted says that they are part of this launch.
static int launch_gemm_lower(gdml_ctx* ctx, hipStream_t st, double* A, int64_t ld, const PlanLowerLaunch& L, int ready_target) {
  const PlanSeg &u = L.upd, &s2 = L.second;
  if (u.M <= 0 || u.N <= 0 || u.K <= 0) return GDML_OK;  // (the plan asks for none: chol.fused_min_rows is clamped there)
  const double* P = A + u.origin * ld + u.a_col0;
  GemmArgs g = gemm_args(P, ld, P, ld, A + u.origin * ld + u.origin, ld, u.M, u.N, u.K, 1);
  g.col0_first = L.col0_first;
  g.diagA = A + L.diag0 * ld + L.diag0; g.diag_nbw = L.diag_nbw; g.diag_off = L.diag0; g.diag_info = ctx->d_info;
  if (L.counted) { g.ready = ctx->d_info + 6; g.ready_target = ready_target; g.ready_rows = L.diag_nbw * 64 / GT; }
  const int64_t n_super_all = g.n_super;
  plan_lower_range(L, &g.s_begin, &g.n_super);
  const double part = (double)(g.n_super - g.s_begin) / (double)n_super_all;  // share of the super-tile list in this launch
  const TileSchedEntry* te = nullptr;
  if (ctx_opt(ctx, "gemm.balance", 1) != 0) GDML_TRY(tile_sched_get(ctx, st, L, &te));
  const int64_t blocks = te ? gemm_use_list(&g, te, L.launch) : (g.n_super - g.s_begin + 7) / 8 * 512;
  if (L.carries_second && s2.M > 0) {
    g.A2 = g.B2 = A + s2.origin * ld + s2.a_col0; g.C2 = A + s2.origin * ld + s2.origin;
    g.M2 = s2.M; g.N2 = s2.N; g.K2 = s2.K;
    bool compact = false;
    const int lead2 = plan_second_blocks(s2.M, s2.N, &compact);
    g.tiles2 = (int)(ceil_div(s2.M, GT) * ceil_div(s2.N, GT));
    if (te && compact) { g.tiles2 = lead2; g.second_compact = 1; }  // no empty workgroups in front of a balanced list either
  }
  // algorithmic flops: a balanced list counts the tiles the launch holds, the super-tile enumeration its share of the list,
  // a launch whose range is the whole list M (M + 1) K either way.  (Of two launches that is the first one where the update
  // has at most 8 tile rows; the second then reports the list's rest once more, 2 K flops too many where a carried row
  // stands alone in the last tile row.  Kept as it was: tests/test_chol_launch_stats_gpu.py holds the recorded counts.)
  const double flops = (te && part < 1.0) ? tile_sched_flops(te->S, L.launch, u.M, u.K, g.tiles_m, GT)
                                          : part * ((double)u.M * (double)(u.M + 1) * (double)u.K);
  // the fused launches (trailing update + diagonal-block workgroup) are the dominant kernel: timed under their own name
  return gemm_issue(ctx, st, gemm_nt_sub_diag_kernel, blocks + 1 + g.tiles2, g, "gemm_nt_sub_diag",
                    flops + 2.0 * (double)g.M2 * (double)g.N2 * (double)g.K2);
}

int launch_gemm_nt_sub(gdml_ctx* ctx, hipStream_t st, const double* A, int64_t lda, const double* B, int64_t ldb, double* C,
                       int64_t ldc, int64_t M, int64_t N, int64_t K, int lower) {
  return launch_gemm_plain(ctx, st, A, lda, B, ldb, C, ldc, M, N, K, lower, nullptr, false);
}

int launch_gemm_nt_neg(gdml_ctx* ctx, hipStream_t st, const double* A, int64_t lda, const double* B, int64_t ldb,
                       double* C, int64_t ldc, int64_t M, int64_t N, int64_t K) {  // C = -A B^T, C not read
  return launch_gemm_plain(ctx, st, A, lda, B, ldb, C, ldc, M, N, K, 0, nullptr, true);
}

int launch_gemm_nt_sub_cyclic(gdml_ctx* ctx, hipStream_t st, const double* A, int64_t lda, const double* B, int64_t ldb,
                              double* C, int64_t ldc, int64_t M, int64_t N, int64_t K, const CyclicLower& cyc) {
  return launch_gemm_plain(ctx, st, A, lda, B, ldb, C, ldc, M, N, K, 0, &cyc, false);
}

// ------------------------------------------------------------------------------------------
// potrf on a w x w (w <= 64) diagonal block, in place (lower).  ONE wavefront: lane r keeps row r of
// the block in registers (fully unrolled right-looking elimination, no barriers); per step the
// scaled column is exchanged through a 64-entry LDS vector (broadcast reads).  Entries above the
// diagonal are scratch.  info (device int): first failing pivot, global 1-based (LAPACK dpotrf).
// ------------------------------------------------------------------------------------------
// One wavefront factors the 64 x 64 tile in T (pitch 65, identity padding outside w x w) in registers: lane = row.
// Returns 0 or the 1-based index of the first non-positive pivot.  Right-looking elimination blocked by 8 columns (round 4;
// bit-identical to the rounds 1-3 form, which sent every scaled column through LDS and waited for the round trip before any
// entry of the next column -- the next pivot included -- could be updated): the columns of the current 8-block are
// updated from lane broadcasts (v_readlane of the scaled column: no memory on the pivot chain), and the columns right of
// the block get the block's 8 rank-1 updates at once from an LDS copy of the 8 finished columns (cb: 64 rows x 8,
// broadcast 16-byte reads).  1/sqrt(d): hardware estimate + two Newton steps (full double precision), then one multiply
// per lane instead of a correctly rounded sqrt and a division on the 64-step critical path.
__device__ __forceinline__ double readlane_f64(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int potrf64_wave(double* T, double* cb /* 64 x 8 */, int lane) {
  double row[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) row[c] = T[lane * 65 + c];
  int fail = 0;
#pragma unroll
  for (int jb = 0; jb < 8; ++jb) {
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int j = 8 * jb + jj;
      const double d = readlane_f64(row[j], j);
      if (!(d > 0.0) && fail == 0) fail = j + 1;
      double ri = __builtin_amdgcn_rsq(d);
      ri = ri * (1.5 - 0.5 * d * ri * ri);
      ri = ri * (1.5 - 0.5 * d * ri * ri);
      const double lr = row[j] * ri;  // lane r: L[r][j] (lane j: d * ri = the pivot's square root; lanes r < j: scratch)
      row[j] = lr;
#pragma unroll
      for (int c = j + 1; c < 8 * jb + 8; ++c) row[c] -= lr * readlane_f64(lr, c);
    }
    if (jb < 7) {
      d2* wr = reinterpret_cast<d2*>(cb + lane * 8);
#pragma unroll
      for (int k = 0; k < 4; ++k) wr[k] = (d2){row[8 * jb + 2 * k], row[8 * jb + 2 * k + 1]};
      __builtin_amdgcn_s_waitcnt(0xc07f);
      // 4 columns at a time, the 8 rank-1 updates applied across them (k outer): four independent multiply-add chains
      // (column by column the compiler emits 8 dependent multiply-adds behind each batch of reads and a lone wavefront
      // pays the full instruction latency 1792 times; 8 columns at a time need > 256 registers: copies through AGPRs)
#pragma unroll
      for (int c0 = 8 * jb + 8; c0 < 64; c0 += 4) {
        d2 l[4][4];
        double v[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const d2* rd = reinterpret_cast<const d2*>(cb + (c0 + g) * 8);
#pragma unroll
          for (int q = 0; q < 4; ++q) l[g][q] = rd[q];
          v[g] = row[c0 + g];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
          for (int g = 0; g < 4; ++g) v[g] -= row[8 * jb + k] * ((k & 1) ? l[g][k >> 1].y : l[g][k >> 1].x);
#pragma unroll
        for (int g = 0; g < 4; ++g) row[c0 + g] = v[g];
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);  // the reads of this block are done before the next block overwrites cb
    }
    __builtin_amdgcn_sched_barrier(0);  // keeps the scheduler from hoisting later blocks' work (and its registers) up here
  }
#pragma unroll
  for (int c = 0; c < 64; ++c) T[lane * 65 + c] = row[c];
  __builtin_amdgcn_s_waitcnt(0xc07f);
  return fail;
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): compile-time expansion of a loop body
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// DPP moves of a double (both halves): quad broadcast of lane q, row shifts
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double quad_bcast(double v, int q) {
  switch (q) {
    case 0: return dpp_mov<0x00>(v);
    case 1: return dpp_mov<0x55>(v);
    case 2: return dpp_mov<0xaa>(v);
    default: return dpp_mov<0xff>(v);
  }
}

// Exact substitution x <- x L^-T of one 64-column block for a row held by 8 threads (thread sq owns the columns k = sq mod 8
// in t[0..7]); Lt = L^T with pitch lp and rinv = 1 / diag(L) in LDS.  What this costs is its 64-step dependent chain, so
// the solved entry travels by DPP (quad broadcast, then a 4-lane row shift into the row's other quad: VALU latency instead
// of an LDS permute round trip), the L values of column c + 1 are fetched from LDS while column c is applied, and the
// column steps are expanded at compile time (a 64-trip loop of this size is only partially unrolled even under
// #pragma unroll, which turns t[c >> 3] into a dynamically indexed register array).
template <int LP>
__device__ __forceinline__ void subst64_row8(double (&t)[8], const double* __restrict__ Lt, const double* __restrict__ rinv,
                                             int sq) {
  double ln[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ln[i] = Lt[sq + 8 * i];
  double rn = rinv[0];
  auto column = [&](auto cc) __attribute__((always_inline)) {
    constexpr int c = decltype(cc)::value;
    constexpr int qc = c & 7, ic = c >> 3;
    double lc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) lc[i] = ln[i];
    const double rc = rn;
    if constexpr (c + 1 < 64) {
      rn = rinv[c + 1];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (i >= ((c + 1) >> 3)) ln[i] = Lt[(c + 1) * LP + sq + 8 * i];
    }
    const double xq = quad_bcast(t[ic] * rc, qc & 3);                      // lane (qc & 3) of the own quad
    const double xo = (qc < 4) ? dpp_mov<0x114>(xq) : dpp_mov<0x104>(xq);  // the other quad's: row_shr:4 / row_shl:4
    const double x = ((sq >> 2) == (qc >> 2)) ? xq : xo;
    if (sq == qc) t[ic] = x;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i > ic || (i == ic && sq > qc)) t[i] -= x * lc[i];
    if constexpr ((c & 7) == 7) __builtin_amdgcn_sched_barrier(0);  // bounds the scheduler's hoisting of later columns' reads
  };
  static_for<64>(column);
}

// ------------------------------------------------------------------------------------------
// Diagonal block of a panel, factored by ONE workgroup (256 threads) inside the trailing-update launch.
// The 64-wide step chain (potrf64, rows below by substitution, rank-64 update) of the nb x nb block is a
// dependent sequence of tiny kernels that the hardware does not overlap with a pending GEMM grid from another
// stream (profiles/r02_sched_probe.txt) and that ran ~650 us per panel exposed.  As workgroup 0 of the SYRK launch
// of the PREVIOUS panel -- which never touches these columns -- it is dispatched first and its ~0.5 ms on one CU
// disappear behind the other workgroups' tiles.  Phases talk through global memory (the block is L2 resident);
// all of them are executed by the same workgroup, so __syncthreads() orders them (waves of a workgroup share the
// CU's vector L1).
//   D: top-left of the block (row-major, ld), nbw = nb / 64.  lds: >= 67 KB (aliased onto the GEMM tile buffers).
// ------------------------------------------------------------------------------------------

// 64 x 64 Cholesky (lower, in place in the LDS tile T, pitch 65) by a whole workgroup of 256 threads with 16
// doubles of state per thread (the one-wavefront version keeps a row of 64 per lane, too many registers next to
// the GEMM role's budget): thread (row = tid / 4, q = tid % 4) holds the columns k = q (mod 4) of its row.
// Right-looking; per step the current column goes through a double-buffered LDS vector: one barrier per step.
// Returns 0 or the 1-based index of the first non-positive pivot (same value in every thread).
__device__ __forceinline__ int potrf64_wg(double* T, double* colbuf /* 2 x 64 */, int tid) {
  const int row = tid >> 2, q = tid & 3;
  double a[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = T[row * 65 + q + 4 * i];
  int fail = 0;
#pragma unroll
  for (int j = 0; j < 64; ++j) {
    const int qj = j & 3, ij = j >> 2;
    double* col = colbuf + (j & 1) * 64;
    if (q == qj) col[row] = a[ij];
    __syncthreads();
    const double d = col[j];
    if (!(d > 0.0) && fail == 0) fail = j + 1;
    double ri = __builtin_amdgcn_rsq(d);
    ri = ri * (1.5 - 0.5 * d * ri * ri);
    ri = ri * (1.5 - 0.5 * d * ri * ri);
    const double lr = col[row] * ri;  // L[row][j] (meaningful for row > j)
    if (q == qj) a[ij] = (row == j) ? d * ri : lr;
#pragma unroll
    for (int i = ij; i < 16; ++i) {
      const int c = q + 4 * i;  // columns right of j only
      const double lc = col[c < 64 ? c : 63] * ri;
      if (i > ij || q > qj) a[i] -= lr * lc;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) T[row * 65 + q + 4 * i] = a[i];
  return fail;
}

__device__ __forceinline__ void diag_block_role(double* __restrict__ D, int64_t ld, int nbw, int64_t global_off,
                                             int* __restrict__ info, double* lds) {
  double* T = lds;                   // 64 x 65 (potrf)
  double* Lt = lds + 64 * 65;        // L_jj^T, pitch 65
  double* rinv = Lt + 64 * 65;       // 64
  double* col = rinv + 64;           // 2 x 64
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int srow = tid >> 3, sq = tid & 7;
  const int nb = 64 * nbw;
  for (int jj = 0; jj < nbw; ++jj) {
    const int c0 = 64 * jj;
    double* Ad = D + (int64_t)c0 * ld + c0;
    for (int r = wave; r < 64; r += 4) T[r * 65 + lane] = Ad[(int64_t)r * ld + lane];
    __syncthreads();
    {
      const int fail = potrf64_wg(T, col, tid);
      if (fail != 0 && tid == 0) atomicCAS(info, 0, (int)(global_off + c0 + fail));
    }
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += 256) {
      const int r = e >> 6, c = e & 63;
      const double v = (c <= r) ? T[r * 65 + c] : 0.0;
      Lt[c * 65 + r] = v;
      if (c <= r) Ad[(int64_t)r * ld + c] = v;
      if (c == r) rinv[r] = 1.0 / v;
    }
    __syncthreads();
    // rows below inside the block: x <- x L_jj^-T by exact substitution, 32 rows per pass, 8 threads per row
    // (thread q of a row holds its columns k = q mod 8; same scheme as panel_trsm_kernel)
    const int mrows = nb - c0 - 64;
    for (int base = 0; base < mrows; base += 32) {
      double* xr = D + (int64_t)(c0 + 64 + base + srow) * ld + c0;
      double t[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) t[i] = xr[sq + 8 * i];
      subst64_row8<65>(t, Lt, rinv, sq);
#pragma unroll
      for (int i = 0; i < 8; ++i) xr[sq + 8 * i] = t[i];
    }
    __syncthreads();
    // rank-64 update of the rest of the block, C -= X_r X_c^T with X = columns [c0, c0+64): lower 32 x 32 macro tiles
    // (2 x 2 MFMA tiles, each operand run loaded once for two tiles), one macro tile per wavefront and turn
    const int nt = mrows / 32;
    const int ntiles = nt * (nt + 1) / 2;
    for (int t = wave; t < ntiles; t += 4) {
      int ti = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
      while (ti * (ti + 1) / 2 > t) --ti;
      while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
      const int tj = t - ti * (ti + 1) / 2;
      const int r0 = c0 + 64 + 32 * ti, q0 = c0 + 64 + 32 * tj;
      double* Cp = D + (int64_t)(r0 + lk) * ld + q0 + li;  // C layout of tile (i, j): row = 16 i + lk + 4 r, col = 16 j + li
      d4 acc[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i][j][r] = Cp[(int64_t)(16 * i + 4 * r) * ld + 16 * j];
      const double* Ap = D + (int64_t)(r0 + li) * ld + c0 + 4 * lk;
      const double* Bp = D + (int64_t)(q0 + li) * ld + c0 + 4 * lk;
      d4 a[2][4], bb[2][4];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
          a[i][ch] = *reinterpret_cast<const d4*>(Ap + (int64_t)(16 * i) * ld + 16 * ch);
          bb[i][ch] = *reinterpret_cast<const d4*>(Bp + (int64_t)(16 * i) * ld + 16 * ch);
        }
#pragma unroll
      for (int ch = 0; ch < 4; ++ch)
#pragma unroll
        for (int sidx = 0; sidx < 4; ++sidx)
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[i][ch][sidx], bb[j][ch][sidx], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) Cp[(int64_t)(16 * i + 4 * r) * ld + 16 * j] = acc[i][j][r];
    }
    __syncthreads();
  }
}


// Workgroup 0 of a fused launch waits until `target` tiles of its diagonal block have counted themselves into *ready (they
// are computed by workgroups of the same launch, dispatched right behind this one).  Bounded: a target that can never be
// reached must not hang the GPU (flag ready[1] -> GDML_ERR_HIP).  MAYBE_NONE: ready may be null (the block is complete
// before the launch: nothing to wait for).
template <bool MAYBE_NONE>
__device__ __forceinline__ void wait_for_tiles(int* ready, int target) {
  if (MAYBE_NONE && !ready) return;
  if (threadIdx.x == 0) {
    int spins = 0;
    while (__hip_atomic_load(ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(8);
      if (++spins > (1 << 24)) {
        atomicExch(ready + 1, 1);
        break;
      }
    }
  }
  __syncthreads();
  __threadfence();
}

// Trailing update + (workgroup 0) the next panel's diagonal block.
__global__ void __launch_bounds__(256, 2) gemm_nt_sub_diag_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) double lds[2][2][GT * GPITCH];
  static_assert(sizeof(double) * 2 * 2 * GT * GPITCH >= sizeof(double) * (2 * 64 * 65 + 64 + 128), "LDS of the diagonal role");
  if (blockIdx.x == 0) {
    wait_for_tiles<true>(g.ready, g.ready_target);
    diag_block_role(g.diagA, g.ldc, g.diag_nbw, g.diag_off, g.diag_info, &lds[0][0][0]);
    return;
  }
  gemm_block<false>(g, lds, (int64_t)blockIdx.x - 1);
}

// Composed launch of the deep schedule (tile_sched.h, chol.deep): up to three segments with their own A, B, C, M, N, K; a
// workgroup reads its (segment, ti, tj) from its XCD's list -- ONE scalar load whose address depends on kernel arguments
// only -- and runs the production tile body on it.  The host lists only tiles that exist (lower, inside M x N): nothing is
// decided per tile but which body, as in gemm_block.  Workgroup 0 is the diagonal-block role of gemm_nt_sub_diag_kernel.
struct SegArgs {
  const double* A[3];
  const double* B[3];
  double* C[3];
  int64_t M[3], N[3], K[3];
  int64_t ld;
  const uint32_t* table;  // [8][stride]
  int stride;
  uint64_t cnt[4];        // entries per XCD, 32 bits each
  double* diagA;
  int diag_nbw;
  int64_t diag_off;
  int* diag_info;
  int* ready;
  int ready_target;
};

__global__ void __launch_bounds__(256, 2) gemm_nt_sub_seg_kernel(SegArgs s) {
  __shared__ __attribute__((aligned(16))) double lds[2][2][GT * GPITCH];
  if (blockIdx.x == 0) {
    wait_for_tiles<false>(s.ready, s.ready_target);
    diag_block_role(s.diagA, s.ld, s.diag_nbw, s.diag_off, s.diag_info, &lds[0][0][0]);
    return;
  }
  const int64_t b = (int64_t)blockIdx.x - 1;
  const int x = (int)(b & 7);
  const int64_t pos = b >> 3;
  if (pos >= (int64_t)((s.cnt[x >> 1] >> (32 * (x & 1))) & 0xffffffffu)) return;
  const uint32_t v = __builtin_amdgcn_readfirstlane(s.table[(int64_t)x * s.stride + pos]);
  const int si = TS_SEG_ID(v);
  GemmArgs h;
  h.A = s.A[0]; h.B = s.B[0]; h.C = s.C[0]; h.M = s.M[0]; h.N = s.N[0]; h.K = s.K[0];
  if (si == 1) { h.A = s.A[1]; h.B = s.B[1]; h.C = s.C[1]; h.M = s.M[1]; h.N = s.N[1]; h.K = s.K[1]; }
  if (si == 2) { h.A = s.A[2]; h.B = s.B[2]; h.C = s.C[2]; h.M = s.M[2]; h.N = s.N[2]; h.K = s.K[2]; }
  h.lda = h.ldb = h.ldc = s.ld;
  const int64_t row0 = TS_SEG_TI(v) * GT, col0 = TS_SEG_TJ(v) * GT;
  const bool aligned = ((reinterpret_cast<uintptr_t>(h.A) | reinterpret_cast<uintptr_t>(h.B)) & 15) == 0 && (s.ld % 2 == 0);
  const bool full = (row0 + GT <= h.M) && (col0 + GT <= h.N) && ((h.K & (GBK - 1)) == 0) && aligned;
  if (full)
    gemm_tile_body<true, false>(h, lds, row0, col0);
  else
    gemm_tile_body<false, false>(h, lds, row0, col0);
  if (TS_SEG_COUNTED(v)) {  // publish the tile (release: every thread's stores, then one count)
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(s.ready, 1);
  }
}

__global__ void __launch_bounds__(64) potrf64_kernel(double* __restrict__ A, int64_t ld, int w,
                                                     int64_t global_off, int* __restrict__ info) {
  __shared__ __attribute__((aligned(16))) double T[64 * 65];
  __shared__ __attribute__((aligned(16))) double col[64 * 8];
  const int lane = threadIdx.x;
  // coalesced load into LDS, identity padding outside the w x w block; all 64 row loads in flight at once (clamped
  // addresses + selects: as a loop around a conditional load each row waited for its own round trip, ~50 of ~80 us)
  {
    double tv[64];
    const int lc = lane < w ? lane : w - 1;
#pragma unroll
    for (int r = 0; r < 64; ++r) tv[r] = A[(int64_t)(r < w ? r : w - 1) * ld + lc];
#pragma unroll
    for (int r = 0; r < 64; ++r) T[r * 65 + lane] = (r < w && lane < w) ? tv[r] : ((r == lane) ? 1.0 : 0.0);
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  const int fail = potrf64_wave(T, col, lane);
  if (fail != 0 && fail <= w && lane == 0) atomicCAS(info, 0, (int)(global_off + fail));
  for (int r = 0; r < w; ++r)
    if (lane <= r && lane < w) A[(int64_t)r * ld + lane] = T[r * 65 + lane];
}

// Fused step of the panel factorisation: every workgroup factors the diagonal block itself (one wavefront,
// redundantly -- cheaper than a separate launch on the panel's dependent chain) and then solves its 256 rows
// below against it.  The diagonal block cannot be written back in place by this launch (other workgroups are
// still reading the unfactored block), so workgroup 0 saves L to `Lsave` and the NEXT launch of the chain (or
// writeback_block_kernel at the end of the panel) stores it: nothing reads a factored diagonal block again
// before the triangular solves.
__global__ void __launch_bounds__(256) potrf_trsm64_kernel(double* __restrict__ A, double* __restrict__ X,
                                                           int64_t ld, int w, int64_t m, int64_t global_off,
                                                           int* __restrict__ info, double* __restrict__ Lsave,
                                                           const double* __restrict__ Lprev,
                                                           double* __restrict__ Aprev, int wprev) {
  __shared__ __attribute__((aligned(16))) double T[64 * 65];
  __shared__ __attribute__((aligned(16))) double Ls[64 * 64];  // L^T (row c = column c of L)
  __shared__ __attribute__((aligned(16))) double col[64 * 8];
  __shared__ double rinv[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // Every global load of this prologue is issued before the first one is used (clamped addresses + selects, no branches
  // around loads): as loops with a conditional load inside, the 16 rows of the block per wavefront and the 16 entries per
  // thread of the deferred write-back each waited for their own round trip -- ~30 of the kernel's ~50 us at the head of
  // every 64-column step of the panel chain (profiles/r04_step_chain.txt).
  double pv[16];
  const bool wb = blockIdx.x == 0 && Lprev != nullptr;  // deferred write-back of the previous diagonal block
  if (wb) {
#pragma unroll
    for (int i = 0; i < 16; ++i) pv[i] = Lprev[tid + 256 * i];
  }
  {
    double tv[16];
    const int lc = lane < w ? lane : w - 1;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = wave + 4 * i;
      tv[i] = A[(int64_t)(r < w ? r : w - 1) * ld + lc];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {  // identity padding outside the w x w block
      const int r = wave + 4 * i;
      T[r * 65 + lane] = (r < w && lane < w) ? tv[i] : ((r == lane) ? 1.0 : 0.0);
    }
  }
  if (wb) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = tid + 256 * i, r = e >> 6, c = e & 63;
      if (r < wprev && c <= r) Aprev[(int64_t)r * ld + c] = pv[i];
    }
  }
  // this thread's row of the strip: requested here, needed after the factorisation (row-per-thread accesses are 64
  // separate 16-byte segments per instruction; measured neutral at n = 6300, -1 ms at n = 63 000)
  const int64_t r = (int64_t)blockIdx.x * 256 + tid;
  double* xr = X + (r < m ? r : m - 1) * ld;
  double x[64];
  const bool al16 = ((reinterpret_cast<uintptr_t>(xr) & 15) == 0) && (w == 64);
  if (al16) {
#pragma unroll
    for (int c = 0; c < 64; c += 2) {
      d2 v = *reinterpret_cast<const d2*>(xr + c);
      x[c] = v.x;
      x[c + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int c = 0; c < 64; ++c) x[c] = (c < w) ? xr[c] : 0.0;
  }
  __syncthreads();
  if (wave == 0) {
    const int fail = potrf64_wave(T, col, lane);
    if (blockIdx.x == 0 && fail != 0 && fail <= w && lane == 0) atomicCAS(info, 0, (int)(global_off + fail));
  }
  __syncthreads();
  for (int e = tid; e < 64 * 64; e += 256) {
    const int r = e >> 6, c = e & 63;
    const double v = (c <= r) ? T[r * 65 + c] : 0.0;  // lower triangle incl. diagonal; identity padding kept
    if (blockIdx.x == 0) Lsave[e] = v;
    if (r == c) rinv[r] = 1.0 / v;
  }
  for (int e = tid; e < 64 * 64; e += 256) {  // L^T: consecutive threads read a column of T (pitch 65), write a row of Ls
    const int c = e >> 6, r = e & 63;
    Ls[e] = (c <= r) ? T[r * 65 + c] : 0.0;
  }
  __syncthreads();
  if (r >= m) return;
  // right-looking substitution: the same multiply-adds in the same order for every entry as a left-looking row loop, but the
  // dependent chain is one multiply-add + one multiply per column instead of the whole dot product (c terms)
#pragma unroll
  for (int c = 0; c < 64; ++c) {
    const double xc = x[c] * rinv[c];
    x[c] = xc;
    const double* Lc = Ls + c * 64;  // L[c'][c], c' = 0..63
    if ((c + 1) & 1) {  // c + 1 odd: one single entry, then aligned pairs
      if (c + 1 < 64) x[c + 1] -= xc * Lc[c + 1];
#pragma unroll
      for (int k = c + 2; k < 64; k += 2) {
        const d2 l = *reinterpret_cast<const d2*>(Lc + k);
        x[k] -= xc * l.x;
        x[k + 1] -= xc * l.y;
      }
    } else {
#pragma unroll
      for (int k = c + 1; k < 64; k += 2) {
        const d2 l = *reinterpret_cast<const d2*>(Lc + k);
        x[k] -= xc * l.x;
        x[k + 1] -= xc * l.y;
      }
    }
  }
  if (al16) {
#pragma unroll
    for (int c = 0; c < 64; c += 2) {
      d2 v = {x[c], x[c + 1]};
      *reinterpret_cast<d2*>(xr + c) = v;
    }
  } else {
#pragma unroll
    for (int c = 0; c < 64; ++c)
      if (c < w) xr[c] = x[c];
  }
}

__global__ void __launch_bounds__(256) writeback_block_kernel(const double* __restrict__ Lprev,
                                                              double* __restrict__ Aprev, int64_t ld, int wprev) {
  double pv[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) pv[i] = Lprev[threadIdx.x + 256 * i];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int e = threadIdx.x + 256 * i, r = e >> 6, c = e & 63;
    if (r < wprev && c <= r) Aprev[(int64_t)r * ld + c] = pv[i];
  }
}

// ------------------------------------------------------------------------------------------
// X[r, 0:w] <- X[r, 0:w] * L^-T for m rows (L = w x w lower block at Ld, w <= 64).  Exact forward
// substitution per row (no explicit inverse): one thread owns one row, holds it in registers
// (fully unrolled), L is broadcast from LDS.  x_c = (x_c - sum_{k<c} x_k L[c][k]) / L[c][c].
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) trsm64_kernel(const double* __restrict__ Ld,
                                                     double* __restrict__ X, int64_t ld, int w,
                                                     int64_t m, int64_t ldl) {
  __shared__ __attribute__((aligned(16))) double Ls[64 * 64];
  const int tid = threadIdx.x;
  for (int e = tid; e < 64 * 64; e += 256) {
    int r = e >> 6, c = e & 63;
    double v = (r == c) ? 1.0 : 0.0;  // identity padding for w < 64
    if (r < w && c < w && c <= r) v = Ld[r * ldl + c];
    Ls[e] = v;
  }
  __syncthreads();
  __shared__ double rinv[64];  // reciprocals of the diagonal: 64 divisions per workgroup instead of 64 per row
  if (tid < 64) rinv[tid] = 1.0 / Ls[tid * 64 + tid];
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 256 + tid;
  if (r >= m) return;
  double* xr = X + r * ld;
  double x[64];
  const bool al16 = ((reinterpret_cast<uintptr_t>(xr) & 15) == 0) && (w == 64);
  if (al16) {
#pragma unroll
    for (int c = 0; c < 64; c += 2) {
      d2 v = *reinterpret_cast<const d2*>(xr + c);
      x[c] = v.x;
      x[c + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int c = 0; c < 64; ++c) x[c] = (c < w) ? xr[c] : 0.0;
  }
#pragma unroll
  for (int c = 0; c < 64; ++c) {
    double s = x[c];
#pragma unroll
    for (int k = 0; k < c; ++k) s -= x[k] * Ls[c * 64 + k];
    x[c] = s * rinv[c];
  }
  if (al16) {
#pragma unroll
    for (int c = 0; c < 64; c += 2) {
      d2 v = {x[c], x[c + 1]};
      *reinterpret_cast<d2*>(xr + c) = v;
    }
  } else {
#pragma unroll
    for (int c = 0; c < 64; ++c)
      if (c < w) xr[c] = x[c];
  }
}

// ------------------------------------------------------------------------------------------
// Row-local panel solve:  X[r, 0:nb] <- X[r, 0:nb] * L^-T  for m rows, L = nb x nb lower (already factored
// diagonal block of the panel), nb = 64 * nbw <= 512.  Replaces the 8 x (trsm64 + K=64 GEMM over the whole
// panel strip) of the panel chain by ONE launch in which every workgroup finishes its own 32 rows: the strip
// is read once and written once instead of eight read-modify-write passes, and the products run on the MFMA pipe.
//
// Workgroup = 32 rows, 4 wavefronts.  The 32 x nb strip lives in REGISTERS in MFMA C-layout: wavefront w owns
// the 64-column blocks {w, 7 - w} (each block 2 x 4 tiles of 16 x 16) -- the right-looking update work of
// block c is c block products, so every wavefront does 7.  Step jj:
//   (1) the owner of block jj writes its (fully updated) block to LDS in row-major form;
//   (2) exact substitution with the 64 x 64 diagonal block L_jj (no explicit inverse, cond(K) ~ 1/lam): 8 threads
//       per row, thread q holds the columns k = q (mod 8); column by column the solved entry is broadcast inside
//       the 8-lane group and the remaining entries are updated (right-looking: independent FMAs); L_jj^T from LDS;
//   (3) the solved block goes to global memory and stays in LDS as the A operand of
//   (4) acc_c -= X_jj * L[c, jj]^T for the blocks c > jj of every wavefront: v_mfma_f64_16x16x4_f64, B operand
//       straight from global memory (L is 2 MB at most and L2 resident).  Both operands are fetched as 32-byte
//       runs (4 consecutive k per lane): MFMA step s of a 16-deep chunk contracts k = 4 (lane >> 4) + s, the same
//       bijection on both sides.
// LDS 50 KB, ~200 VGPRs: two workgroups per CU, the second one covers the substitution phases of the first.
// ------------------------------------------------------------------------------------------
#define PT_ROWS 32
#define PT_SP 66   // pitch of the row-major block in LDS (doubles): 16-byte aligned rows, 16-lane b128 reads conflict-free
#define PT_LP 65   // pitch of L_jj^T

#define PT_TB (64 * PT_LP + 64)  // per 64-block image in the prep buffer: L_jj^T (pitch PT_LP) followed by 1 / diag

// One workgroup per 64 x 64 diagonal block of L: transposed copy (zero above the diagonal) + reciprocal pivots, in the
// exact LDS image of panel_trsm_kernel.  Every row block of the solve used to redo this transpose (and its 64 divisions)
// per step; it was 13 of the kernel's 53 ms (profiles/r02_panel_trsm_breakdown.txt).
__global__ void __launch_bounds__(256) panel_trsm_prep_kernel(const double* __restrict__ L, int64_t ldl,
                                                              double* __restrict__ Tb) {
  const int jj = blockIdx.x, tid = threadIdx.x;
  double* T = Tb + (int64_t)jj * PT_TB;
  double lv[16];  // all 16 loads of a thread in flight at once (a conditional load in the loop waits for each round trip)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int e = tid + 256 * i;
    lv[i] = L[(int64_t)(jj * 64 + (e >> 6)) * ldl + jj * 64 + (e & 63)];
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int e = tid + 256 * i, r = e >> 6, c = e & 63;  // L_jj[r][c], c <= r
    const double v = (c <= r) ? lv[i] : 0.0;
    T[c * PT_LP + r] = v;
    if (r == c) T[64 * PT_LP + r] = 1.0 / v;
  }
  if (tid < 64) T[tid * PT_LP + 64] = 0.0;  // pitch padding (copied along, never read)
}

template <bool ABL>
__global__ void __launch_bounds__(256, 2) panel_trsm_kernel(const double* __restrict__ Tb, const double* __restrict__ L, int64_t ldl,
                                                            double* __restrict__ X, int64_t ld, int nbw, int64_t m, int dbg) {
  __shared__ __attribute__((aligned(16))) double S[PT_ROWS * PT_SP];
  __shared__ __attribute__((aligned(16))) double Lt[PT_TB];
  double* const rinv = Lt + 64 * PT_LP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * PT_ROWS;
  // ---- strip into registers (C layout: row = lk + 4 r + 16 i, col = li + 16 j); two separately named register
  // blocks (an array indexed by the owner test would be demoted to scratch memory)
  d4 accA[2][4], accB[2][4];
  const int blkA = wave, blkB = 7 - wave;
  // every load of the strip is issued before the first use: clamped addresses + selects, no branch around a load (with the
  // `blk < nbw` test inside the tile loop the compiler emitted 16 branches, each 4 loads + s_waitcnt vmcnt(0): 16 memory
  // round trips per workgroup before the first step)
  auto load_block = [&](d4 (&acc)[2][4], int blk) {
    const bool have = blk < nbw && !(ABL && (dbg & 8));
    const double* pb = X + (have ? blk : 0) * 64 + li;
    double w[2][4][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t gr = row0 + 16 * i + lk;
      // rows past m read row m-1 (clamped index + select instead of predicated loads)
      const int64_t r0 = gr < m ? gr : m - 1, r1 = gr + 4 < m ? gr + 4 : m - 1;
      const int64_t r2 = gr + 8 < m ? gr + 8 : m - 1, r3 = gr + 12 < m ? gr + 12 : m - 1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double* pc = pb + 16 * j;
        w[i][j][0] = pc[r0 * ld];  // (non-temporal loads of the strip: measured neutral, profiles/r04_gemm_peel_stagger_ab.txt)
        w[i][j][1] = pc[r1 * ld];
        w[i][j][2] = pc[r2 * ld];
        w[i][j][3] = pc[r3 * ld];
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t gr = row0 + 16 * i + lk;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = (d4){(have && gr < m) ? w[i][j][0] : 0.0, (have && gr + 4 < m) ? w[i][j][1] : 0.0,
                         (have && gr + 8 < m) ? w[i][j][2] : 0.0, (have && gr + 12 < m) ? w[i][j][3] : 0.0};
    }
  };
  load_block(accA, blkA);
  load_block(accB, blkB);

  auto to_lds = [&](const d4 (&acc)[2][4]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) S[(16 * i + lk + 4 * r) * PT_SP + 16 * j + li] = acc[i][j][r];
  };
  auto update = [&](d4 (&acc)[2][4], int c, int jj) {
    const double* Lc = L + (int64_t)(c * 64 + li) * ldl + jj * 64 + 4 * lk;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {  // 16-deep chunks of the 64 contraction indices
      d4 a[2], bb[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const d4*>(&S[(16 * i + li) * PT_SP + 16 * ch + 4 * lk]);
#pragma unroll
      for (int j = 0; j < 4; ++j) bb[j] = *reinterpret_cast<const d4*>(Lc + (int64_t)(16 * j) * ldl + 16 * ch);
#pragma unroll
      for (int sidx = 0; sidx < 4; ++sidx)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)  // acc -= a b^T  ==  acc += (-a) b^T
            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[i][sidx], bb[j][sidx], acc[i][j], 0, 0, 0);
    }
  };

  for (int jj = 0; jj < nbw; ++jj) {
    // (1) owner's block -> LDS row-major; L_jj^T and reciprocal diagonal -> LDS
    if (jj < 4) {
      if (wave == jj) to_lds(accA);
    } else {
      if (wave == 7 - jj) to_lds(accB);
    }
    if (!(ABL && (dbg & 4))) {  // L_jj^T and reciprocal pivots: straight copy of the prepared image
      const d2* src = reinterpret_cast<const d2*>(Tb + (int64_t)jj * PT_TB);
      d2* dst = reinterpret_cast<d2*>(Lt);
#pragma unroll
      for (int k = 0; k < (PT_TB / 2 + 255) / 256; ++k) {
        const int e = tid + 256 * k;
        if (e < PT_TB / 2) dst[e] = src[e];
      }
    }
    __syncthreads();
    // (2) substitution: x_c = t_c / L[c][c];  t_k -= x_c L[k][c] for k > c.  8 threads per row (subst64_row8)
    if (!ABL || !(dbg & 1)) {
      const int srow = tid >> 3, sq = tid & 7;
      double t[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) t[i] = S[srow * PT_SP + sq + 8 * i];
      if (!(ABL && (dbg & 32))) subst64_row8<PT_LP>(t, Lt, rinv, sq);
      const int64_t gr = row0 + srow;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        S[srow * PT_SP + sq + 8 * i] = t[i];
        if (gr < m && !(ABL && (dbg & 16))) X[gr * ld + jj * 64 + sq + 8 * i] = t[i];
      }
    }
    __syncthreads();
    // (4) right-looking update of the blocks c > jj this wavefront owns
    if (!ABL || !(dbg & 2)) {
      if (blkA > jj && blkA < nbw) update(accA, blkA, jj);
      if (blkB > jj && blkB < nbw) update(accB, blkB, jj);
    }
    __syncthreads();  // S and Lt are rewritten by the next step
  }
}

// L: nb x nb lower block (leading dimension ldl; 0 = the same matrix as X), X: m rows of leading dimension ld
int launch_panel_trsm(gdml_ctx* ctx, hipStream_t st, const double* L, double* X, int64_t ld, int nb, int64_t m,
                      int64_t ldl) {
  if (m <= 0) return GDML_OK;
  const int dbg = ctx_opt_i(ctx, "trsm.debug", 0);  // timing-only ablation bits: 1 no substitution, 2 no MFMA update,
                                                    // 4 no L_jj staging, 8 no strip load, 16 no stores
  double* Tb = nullptr;
  GDML_TRY(ctx_slot(ctx, SLOT_PANEL_TRSM, (int64_t)8 * PT_TB * 8, &Tb));
  const int slot = (st == (ctx->kt_stream ? ctx->kt_stream : ctx->stream)) ? ktime_begin(ctx) : -1;
  hipLaunchKernelGGL(panel_trsm_prep_kernel, dim3((unsigned)(nb / 64)), dim3(256), 0, st, L, ldl > 0 ? ldl : ld, Tb);
  if (dbg)
    hipLaunchKernelGGL(panel_trsm_kernel<true>, dim3((unsigned)ceil_div(m, PT_ROWS)), dim3(256), 0, st, Tb, L, ldl > 0 ? ldl : ld,
                       X, ld, nb / 64, m, dbg);
  else
    hipLaunchKernelGGL(panel_trsm_kernel<false>, dim3((unsigned)ceil_div(m, PT_ROWS)), dim3(256), 0, st, Tb, L, ldl > 0 ? ldl : ld,
                       X, ld, nb / 64, m, 0);
  ctx->launch_counter++;
  ktime_end(ctx, slot, "panel_trsm", (double)m * (double)nb * (double)nb);
  ctx->launch_counter++;
  HIP_CHECK(ctx, hipGetLastError());
  return GDML_OK;
}

int launch_trsm64(gdml_ctx* ctx, hipStream_t st, const double* Ld, double* X, int64_t ld, int w,
                  int64_t m, int64_t ldl) {
  if (m <= 0) return GDML_OK;
  hipLaunchKernelGGL(trsm64_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, st, Ld, X, ld, w, m, ldl > 0 ? ldl : ld);
  ctx->launch_counter++;
  HIP_CHECK(ctx, hipGetLastError());
  return GDML_OK;
}

// Rank-64 update inside the panel chain:  C[m x ncols] -= A[m x 64] B[ncols x 64]^T with a handful of tiles (the rest of an
// nb x nb diagonal block after one 64-column step: m, ncols <= 448).  The 128 x 128 GEMM tile kernel is the wrong tool
// there: most tiles are ragged (its guarded path loads element-wise and runs a load-subtract-store epilogue in four
// serialised batches) and a launch took 20-60 us for < 30 MFLOP, on the dependent chain of every panel.  Here one wavefront
// owns a 32 x 32 tile (2 x 2 MFMA tiles), both operands come straight from global memory (L2) in MFMA layout as 32-byte
// runs and ALL loads of the tile -- C included -- are issued before the first use: one memory round trip + 64 MFMAs.
// Ragged edges: clamped row indices on the loads, guarded stores.  skip_upper: tiles strictly above the diagonal are not
// computed (C's origin lies on the matrix diagonal; the strict upper triangle is scratch).
__global__ void __launch_bounds__(256) rank64_update_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                            double* __restrict__ C, int64_t ld, int m, int ncols,
                                                            int skip_upper) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int tn = (ncols + 31) >> 5;
  const int t = blockIdx.x * 4 + wave;
  const int ti = t / tn, tj = t - ti * tn;
  if (32 * ti >= m) return;
  if (skip_upper && tj > ti) return;
  const int r0 = 32 * ti, q0 = 32 * tj;
  d4 acc[2][2], a[2][4], bb[2][4];
  int crow[2][4], ccol[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) ccol[j] = q0 + 16 * j + li;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) crow[i][r] = r0 + 16 * i + lk + 4 * r;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ra = r0 + 16 * i + li, rb = q0 + 16 * i + li;
    const double* Ap = A + (int64_t)(ra < m ? ra : m - 1) * ld + 4 * lk;
    const double* Bp = B + (int64_t)(rb < ncols ? rb : ncols - 1) * ld + 4 * lk;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      a[i][ch] = *reinterpret_cast<const d4*>(Ap + 16 * ch);
      bb[i][ch] = *reinterpret_cast<const d4*>(Bp + 16 * ch);
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = crow[i][r] < m ? crow[i][r] : m - 1, cc = ccol[j] < ncols ? ccol[j] : ncols - 1;
        acc[i][j][r] = C[(int64_t)rr * ld + cc];
      }
#pragma unroll
  for (int ch = 0; ch < 4; ++ch)
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[i][ch][sidx], bb[j][ch][sidx], acc[i][j], 0, 0, 0);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (crow[i][r] < m && ccol[j] < ncols) C[(int64_t)crow[i][r] * ld + ccol[j]] = acc[i][j][r];
}

// ---- the factorisation's plan (tile_sched.h).  A plan with composed launches is cached per (n, rows, options) together with
// its launch tables, which live in a device allocation of their own, sized from the plan (2.8 MB at n = 63 000, 36 MB at
// 150 000); the few most recent ones are kept.  A plan without composed launches (every small factorisation) is a short list
// of operations, built per call and not kept.
struct CholPlanEntry {
  CholPlan plan;
  uint32_t* block = nullptr;         // device tables of all composed launches
  std::vector<const uint32_t*> dev;  // per composed launch: [8][stride]
  std::vector<int> stride;
  ~CholPlanEntry() {
    if (block) (void)hipFree(block);  // (waits for the device: nothing in flight reads the tables any more)
  }
};

static int chol_plan_get(gdml_ctx* ctx, hipStream_t st, int64_t n, int64_t n_rows, CholPlanOpts po, std::shared_ptr<CholPlanEntry>* out) {
  if (!ctx->tile_sched) ctx->tile_sched = new TileSchedCache();
  TileSchedCache* c = ctx->tile_sched;
  const std::array<int64_t, 8> key = {n, n_rows, po.NB, po.OB, po.outer_min_rows, po.fused_min_rows, po.deep, po.deep_min_rows};
  for (auto& kv : c->plans)
    if (kv.first == key) { *out = kv.second; return GDML_OK; }
  auto e = std::make_shared<CholPlanEntry>();
  chol_plan_build(n, n_rows, po, &e->plan);
  *out = e;
  if (e->plan.segs.empty()) return GDML_OK;
  std::vector<uint32_t> host;
  std::vector<size_t> at;
  for (const PlanSegLaunch& L : e->plan.segs) {
    const size_t stride = plan_launch_stride(L);
    at.push_back(host.size());
    e->stride.push_back((int)stride);
    host.resize(host.size() + plan_launch_words(L), 0);
    for (int x = 0; x < 8; ++x) std::copy(L.xcd[x].begin(), L.xcd[x].end(), host.begin() + at.back() + x * stride);
  }
  if (hipMalloc((void**)&e->block, host.size() * 4) != hipSuccess) {
    // no room for the tables beside the matrix: the one-level schedule needs none and computes the same factor
    (void)hipGetLastError();
    e->block = nullptr;
    po.deep = 0;
    e->plan = CholPlan();
    e->stride.clear();
    chol_plan_build(n, n_rows, po, &e->plan);
    return GDML_OK;
  }
  HIP_CHECK(ctx, hipMemcpyAsync(e->block, host.data(), host.size() * 4, hipMemcpyHostToDevice, st));
  HIP_CHECK(ctx, hipStreamSynchronize(st));  // once per plan: the host copy goes out of scope
  for (size_t o : at) e->dev.push_back(e->block + o);
  if (c->plans.size() >= 4) c->plans.erase(c->plans.begin());  // oldest first
  c->plans.emplace_back(key, e);
  return GDML_OK;
}

static int launch_gemm_seg(gdml_ctx* ctx, hipStream_t st, double* A, int64_t ld, const CholPlanEntry& pe, int idx, int ready_target) {
  const PlanSegLaunch& L = pe.plan.segs[idx];
  SegArgs s = {};
  for (int i = 0; i < 3; ++i) {
    const PlanSeg& g = L.seg[i];
    s.A[i] = A + g.origin * ld + g.a_col0;
    s.B[i] = s.A[i];
    s.C[i] = A + g.origin * ld + g.origin;
    s.M[i] = g.M; s.N[i] = g.N; s.K[i] = g.K;
  }
  s.ld = ld;
  s.table = pe.dev[idx];
  s.stride = pe.stride[idx];
  int64_t mx = 0;
  for (int x = 0; x < 8; ++x) {
    const int64_t cnt = (int64_t)L.xcd[x].size();
    s.cnt[x >> 1] |= (uint64_t)cnt << (32 * (x & 1));
    if (cnt > mx) mx = cnt;
  }
  s.diagA = A + L.diag0 * ld + L.diag0;
  s.diag_nbw = L.diag_nbw;
  s.diag_off = L.diag0;
  s.diag_info = ctx->d_info;
  s.ready = ctx->d_info + 6;
  s.ready_target = ready_target;
  const int slot = (st == (ctx->kt_stream ? ctx->kt_stream : ctx->stream)) ? ktime_begin(ctx) : -1;
  hipLaunchKernelGGL(gemm_nt_sub_seg_kernel, dim3((unsigned)(8 * mx + 1)), dim3(256), 0, st, s);
  // the composed launches are trailing-update launches like the paired ones: timed under the same name, flops counted from
  // the tiles they hold; the far tiles' share is kept under a name of its own (launches and flops, no time)
  ktime_end(ctx, slot, "gemm_nt_sub_diag", L.flops);
  if (slot >= 0 && L.far_tiles > 0) {
    KernelStat& k = ctx->kstats["gemm_nt_sub_deep"];
    k.launches += 1;
    k.work += L.far_flops;
  }
  ctx->launch_counter++;
  HIP_CHECK(ctx, hipGetLastError());
  return GDML_OK;
}

// Factor one panel: columns [k0, k0+nb), rows [k0, n), 64-wide sub-steps (potrf_trsm64 / rank-64 update).
int panel_factor_steps(gdml_ctx* ctx, hipStream_t st, double* A, int64_t n, int64_t ld, int64_t k0, int64_t nb);

// Panel = diagonal block (the 64-wide step chain, but only over the nb rows of the block) + ONE row-local solve of
// all rows below; the step chain over the whole strip for ragged or unaligned panels.
static int panel_factor(gdml_ctx* ctx, hipStream_t st, double* A, int64_t n, int64_t ld, int64_t k0,
                        int64_t nb) {
  const int64_t below = n - k0 - nb;
  const bool aligned = (reinterpret_cast<uintptr_t>(A) & 31) == 0 && (ld % 4 == 0) && (k0 % 4 == 0);
  if (nb % 64 == 0 && nb <= 512 && below > 0 && aligned) {
    GDML_TRY(panel_factor_steps(ctx, st, A, k0 + nb, ld, k0, nb));
    return launch_panel_trsm(ctx, st, A + k0 * ld + k0, A + (k0 + nb) * ld + k0, ld, (int)nb, below);
  }
  return panel_factor_steps(ctx, st, A, n, ld, k0, nb);
}

int panel_factor_steps(gdml_ctx* ctx, hipStream_t st, double* A, int64_t n, int64_t ld, int64_t k0,
                       int64_t nb) {
  double* save = nullptr;  // two 64 x 64 slots for the deferred write-back of the diagonal blocks
  GDML_TRY(ctx_slot(ctx, SLOT_PANEL_SAVE, 2 * 4096 * 8, &save));
  const double* Lprev = nullptr;
  double* Aprev = nullptr;
  int wprev = 0, flip = 0;
  for (int64_t jj = 0; jj < nb; jj += 64) {
    const int64_t c0 = k0 + jj;
    const int w = (int)((nb - jj < 64) ? nb - jj : 64);
    double* Ad = A + c0 * ld + c0;
    const int64_t m = n - c0 - w;
    if (m > 0) {
      double* X = A + (c0 + w) * ld + c0;
      double* Lsave = save + flip * 4096;
      hipLaunchKernelGGL(potrf_trsm64_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, st, Ad, X, ld, w, m,
                         c0, ctx->d_info, Lsave, Lprev, Aprev, wprev);
      ctx->launch_counter++;
      Lprev = Lsave;
      Aprev = Ad;
      wprev = w;
      flip ^= 1;
      const int64_t ncols = k0 + nb - (c0 + w);
      if (ncols > 0) {
        // rest of the panel:  C[c0+w:n, c0+w:k0+nb] -= X[c0+w:n, :] X[c0+w:k0+nb, :]^T
        const bool al32 = (reinterpret_cast<uintptr_t>(X) & 31) == 0 && (ld % 4 == 0);
        if (w == 64 && m <= 2048 && al32) {  // a handful of tiles: one wavefront per 32 x 32 tile
          const int tiles = (int)(ceil_div(m, 32) * ceil_div(ncols, 32));
          hipLaunchKernelGGL(rank64_update_kernel, dim3((unsigned)ceil_div(tiles, 4)), dim3(256), 0, st, X, X,
                             A + (c0 + w) * ld + (c0 + w), ld, (int)m, (int)ncols, 1);
          ctx->launch_counter++;
        } else {
          GDML_TRY(launch_gemm_nt_sub(ctx, st, X, ld, X, ld, A + (c0 + w) * ld + (c0 + w), ld, m, ncols, w, 0));
        }
      }
    } else {  // last block of the matrix: flush the pending diagonal block, then factor this one alone
      if (Lprev) {
        hipLaunchKernelGGL(writeback_block_kernel, dim3(1), dim3(256), 0, st, Lprev, Aprev, ld, wprev);
        ctx->launch_counter++;
        Lprev = nullptr;
      }
      hipLaunchKernelGGL(potrf64_kernel, dim3(1), dim3(64), 0, st, Ad, ld, w, c0, ctx->d_info);
      ctx->launch_counter++;
    }
  }
  if (Lprev) {
    hipLaunchKernelGGL(writeback_block_kernel, dim3(1), dim3(256), 0, st, Lprev, Aprev, ld, wprev);
    ctx->launch_counter++;
  }
  return GDML_OK;
}

// n: order of the matrix; n_rows >= n: rows n..n_rows-1 are carried along (right-hand sides stored as extra
// rows: they go through the panel solves and trailing updates, i.e. through the forward substitution)
int chol_factor_device(gdml_ctx* ctx, double* A, int64_t n, int64_t ld, int* info_out, int64_t n_rows) {
  if (n_rows < n) n_rows = n;
  HIP_CHECK(ctx, hipMemsetAsync(ctx->d_info, 0, sizeof(int), ctx->stream));
  // ONE stream; the per-panel flow is in the file header.  The schedule is a pure host function (chol_plan_build,
  // tile_sched.h: panel pairs while the trailing matrix is large, then single fused panels, then the tail; chol.deep = W > 0:
  // far trailing tiles receive a whole block of W columns in one pass that rides in the next block's launches, OP_SEG).  It
  // clamps the options and states every fused launch in full: this loop only turns origins into pointers.
  hipStream_t st = ctx->stream;
  CholPlanOpts po;
  po.NB = (int64_t)ctx_opt(ctx, "chol.nb", 512);  // outer panel width (multiple of 64)
  po.OB = (int64_t)ctx_opt(ctx, "chol.outer", 1024);
  po.outer_min_rows = (int64_t)ctx_opt(ctx, "chol.outer_min_rows", 16384);
  po.fused_min_rows = (int64_t)ctx_opt(ctx, "chol.fused_min_rows", 12288);
  po.deep = (int64_t)ctx_opt(ctx, "chol.deep", 4096);
  po.deep_min_rows = (int64_t)ctx_opt(ctx, "chol.deep_min_rows", 26624);
  std::shared_ptr<CholPlanEntry> pe;
  GDML_TRY(chol_plan_get(ctx, st, n, n_rows, po, &pe));
  HIP_CHECK(ctx, hipMemsetAsync(ctx->d_info + 6, 0, 2 * sizeof(int), ctx->stream));  // tile counter, wait-timeout flag
  for (const CholOp& c : pe->plan.ops) {
    const int64_t k0 = c.k0, nb = c.nb, t0 = c.t0, nb2 = c.nb2, t1 = t0 + nb2;
    const double* P = A + t0 * ld + k0;
    const double* P1 = A + t1 * ld + k0;
    switch (c.kind) {
      case OP_PANEL:  // first panel (nothing to hide its diagonal block behind) and the last one
        GDML_TRY(panel_factor(ctx, st, A, n_rows, ld, t0, nb2));
        break;
      case OP_TRSM:
        GDML_TRY(launch_panel_trsm(ctx, st, A + t0 * ld + t0, A + t1 * ld + t0, ld, (int)nb2, n_rows - t1));
        break;
      case OP_PAIR1:
      case OP_PAIR2:
      case OP_FUSED:
        GDML_TRY(launch_gemm_lower(ctx, st, A, ld, pe->plan.lowers[c.lower], c.ready_target));
        break;
      case OP_SEG:
        GDML_TRY(launch_gemm_seg(ctx, st, A, ld, *pe, c.seg, c.ready_target));
        break;
      case OP_RECT:
        GDML_TRY(launch_gemm_nt_sub(ctx, st, P, ld, P, ld, A + t0 * ld + t0, ld, n_rows - t0, nb2, nb, 0));
        break;
      case OP_TAIL: {
        // tail: the SYRK is too short to hide the single-workgroup block factorisation; the multi-workgroup step chain and
        // the row-local solve of panel k+1 run on the high-priority stream next to the (small) SYRK grid of panel k
        hipStream_t sp = ctx->stream2;
        HIP_CHECK(ctx, hipEventRecord(ctx->ev_la[0], st));
        HIP_CHECK(ctx, hipStreamWaitEvent(sp, ctx->ev_la[0], 0));
        GDML_TRY(panel_factor(ctx, sp, A, n_rows, ld, t0, nb2));
        HIP_CHECK(ctx, hipEventRecord(ctx->ev_la[1], sp));
        GDML_TRY(launch_gemm_nt_sub(ctx, st, P1, ld, P1, ld, A + t1 * ld + t1, ld, n_rows - t1, n - t1, nb, 1));
        HIP_CHECK(ctx, hipStreamWaitEvent(st, ctx->ev_la[1], 0));
        break;
      }
    }
  }
  HIP_CHECK(ctx, hipGetLastError());
  int info8[8] = {0};
  HIP_CHECK(ctx, hipMemcpyAsync(info8, ctx->d_info, sizeof(info8), hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (info8[7] != 0)
    return gdml_fail(ctx, GDML_ERR_HIP, "Cholesky: the diagonal-block workgroup gave up waiting for its tiles (schedule bug)");
  if (info_out) *info_out = info8[0];
  return GDML_OK;
}

// Host-side plan of the Nystroem build and of the stored forms of the preconditioner application: how gram_tn (gram_tn.hip)
// cuts the contraction, which form gdml_nystroem_factor (nystroem.hip) builds, and for precon_apply_device
// (precon_apply.hip) the grids, the template selectors, the layout of SLOT_PRECON_GEMV and the figures booked per call.
// Plain C++ with no HIP include and no gdml_ctx, so that the decision is a value one can print and test without a GPU
// (tests/precon_plan_driver.cpp, tests/test_precon_plan_cpu.py).
#pragma once
#include <stdint.h>

// tile constants of the Gram kernels (gram_tn.hip), which the plan has to respect
constexpr int TT = 128;  // tile edge
constexpr int TBK = 16;  // rows of X per k-tile

// ---- gram_tn: C (m x m, lower tiles) = X^T X over n rows.  Option nys.syrk_split (default 1) cuts the contraction into S row
// ranges of rows_per rows when the tile count is only a few rounds of the chip (why: above syrk_tn_split_kernel); each range
// sums into its own m x ldc image (part_bytes in all).
struct GramSplitPlan {
  int tiles;         // tile rows
  int64_t T;         // lower tiles
  int S;             // row ranges (1: the one-pass kernel, no images)
  int64_t rows_per;  // rows per range, a multiple of TBK when S > 1 (S = 1: n)
  int64_t part_bytes;
};
inline GramSplitPlan gram_split_plan(int64_t n, int64_t m, int64_t ldc, int split_option) {
  GramSplitPlan p;
  p.tiles = (int)((m + TT - 1) / TT);
  p.T = (int64_t)p.tiles * (p.tiles + 1) / 2;
  p.S = 1;
  if (split_option != 0 && p.T < 8192) {
    p.S = (int)((8192 + p.T - 1) / p.T);
    if (p.S > 8) p.S = 8;
    while (p.S > 1 && n / p.S < 8192) --p.S;                                // every range long enough to be worth a tile's prologue
    while (p.S > 1 && (int64_t)p.S * m * ldc * 8 > ((int64_t)2 << 30)) --p.S;  // at most 2 GiB of partial images (measured: no gain beyond)
  }
  p.rows_per = p.S > 1 ? ((n + p.S - 1) / p.S + TBK - 1) / TBK * TBK : n;
  p.part_bytes = p.S > 1 ? (int64_t)p.S * m * ldc * 8 : 0;
  return p;
}

// ---- form of the preconditioner application (option pcg.precon_form):
//   0  the stored n x m fp64 factor, streamed twice per application -- the reference's operator (iterative.py:120-140)
//   1  matrix-free (two kernel mat-vecs + the m x m matrix Z).  Experimental: the same operator to ~1e-8 of its norm, which
//      is NOT enough -- (X X^T - I) v cancels to lam / (sigma + lam) ~ 1e-12 on the dominant subspace, X = K_nm Z is only
//      orthonormal when formed row by row (cond(K_nm) ~ 1e10: |K_nm| |Z| eps ~ 1e-5), and PCG at lam = 1e-10 does not
//      converge with it (profiles/r05_pcg_bisect.txt).  Usable for lam >~ 1e-6; never chosen automatically.
//   3  the factor stored in fp32 + the m x m Gram correction T0 (nystroem.hip): half the bytes per application
//   2  automatic (default): 3 once the factor reaches 1 GiB per rank, else 0 -- every reference-parity fixture of the test
//      suite stays on the reference's form.  The extra build work of form 3 (one more Gram pass over the factor, 2 n m^2
//      flops, ~8 m^3 for T0) is paid back twice: half the bytes per application, and -- the larger effect -- FEWER
//      iterations: the stored factor carries the spectrum 1 - lam / (sigma + lam) of the dominant directions only to ~1e-10
//      (its Gram matrix is off the exact one by that much), which parks PCG on a plateau for hundreds of iterations; T0
//      carries it to ~1e-16 (configs[2]: 861 -> 306 iterations, configs[4]: 2261 -> 841, profiles/r05_precon_forms.txt).
// chunk: rows per rank of the sharded factor (VecLayout::chunk).  Every input is the same on every rank.
inline int choose_precon_form(int option, int64_t chunk, int64_t m) {
  if (option == 0 || option == 1 || option == 3) return option;
  return 8.0 * (double)chunk * (double)m >= (double)((int64_t)1 << 30) ? 3 : 0;
}

// rows of the rounded factor widened per Gram launch of build_f32_form (option pcg.f32_gram_rows, default 2048)
inline int64_t f32_gram_chunk(int64_t option, int64_t n_loc) {
  int64_t chunk = option < 256 ? 256 : option / 16 * 16;
  if (chunk > n_loc) chunk = n_loc > 0 ? n_loc : 1;
  return chunk;
}

// ---- one application of a stored form, (X X^T v - v) / lam (form 0) or (X32 T0 X32^T v - v) / lam (form 3), on this rank's
// n_loc rows: row parts of X^T v, their reduction, [all-reduce], T0 in between (form 3), X t, [all-gather].
struct PreconOpts {
  int gemv_plain;    // pcg.gemv_plain (default 0): plain instead of non-temporal loads of the factor
  int f32_rows_per;  // pcg.f32_rows_per (default 1024): rows per part of X32^T v
  int f32_rw;        // pcg.f32_rw (default 4): rows per wavefront of X32 u
};
struct PreconApplyPlan {
  int form;
  bool nt;               // non-temporal loads: the factor is streamed (25 GB per pass at configs[2]), profiles/r04_gemv_nt_ab.txt
  int rows_per, nparts;  // row parts of X^T v (grid y)
  int rw;                // rows per wavefront of X t: 4 | 2 | 1 (form 0: 1)
  unsigned col_blocks;   // grid x of X^T v: 512 columns per workgroup in fp64, 1024 in fp32
  unsigned row_blocks;   // grid of X t: four wavefronts of rw rows per workgroup
  // SLOT_PRECON_GEMV in doubles: part (nparts x m) at 0, t at an even offset (read in pairs), u behind t (form 3: T0 t,
  // zeroed over its n_u entries so that the pad [m, m4) reads zero)
  int64_t o_t, o_u, n_u, ws_bytes;
  int launches;  // added to launch_counter
  double work;   // bytes of the factor read, handed to ktime_end("precon_gemv")
};
inline PreconApplyPlan precon_apply_plan(int form, int64_t n_loc, int64_t m, int64_t ld, const PreconOpts& o) {
  PreconApplyPlan p;
  const bool f32 = form == 3;
  p.form = form;
  p.nt = o.gemv_plain == 0;
  p.rows_per = f32 ? (o.f32_rows_per < 64 ? 64 : o.f32_rows_per) : 2048;
  p.nparts = (int)((n_loc + p.rows_per - 1) / p.rows_per);
  if (p.nparts < 1) p.nparts = 1;
  p.rw = !f32 ? 1 : o.f32_rw >= 4 ? 4 : o.f32_rw >= 2 ? 2 : 1;
  p.col_blocks = (unsigned)((m + (f32 ? 1024 : 512) - 1) / (f32 ? 1024 : 512));
  p.row_blocks = (unsigned)((n_loc + 4 * p.rw - 1) / (4 * p.rw));
  p.o_t = ((int64_t)p.nparts * m + 1) & ~(int64_t)1;
  p.o_u = p.o_t + (f32 ? ld : m);
  p.n_u = f32 ? ld : 0;
  p.ws_bytes = ((int64_t)p.nparts * m + (f32 ? 2 * ld + 4 : m + 2)) * 8;
  p.launches = f32 ? 5 : 3;
  p.work = f32 ? 2.0 * 4.0 * (double)n_loc * (double)m + 8.0 * (double)m * (double)m : 2.0 * 8.0 * (double)n_loc * (double)m;
  return p;
}

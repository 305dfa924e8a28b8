// Host-side plan of the batched predictor (predict_device_w, predict.hip): which kernel serves a batch, with which template
// selector, grid, row split, LDS and workspace.  Plain C++ with no HIP include and no gdml_ctx, so that the decision is a
// value one can print and test without a GPU (tests/predict_plan_driver.cpp, tests/test_predict_plan_cpu.py).
//
// ROUTING.  D = N (N - 1) / 2 descriptor entries, B queries, MP = M P permuted table rows.  The first line that holds:
//   WIDE  D > 8192, whatever the batch and the options (predict_big_kernel<16> has no registers for a longer row; the GEMM
//         pipeline of predict_wide.hip has no size limit: correct for a single query too, if not tuned for it); or
//         B >= 256, D > 256, predict.wave_only = 0 and (predict.mfma_wide = 2, or predict.mfma_wide = 1 and
//         MP B D >= 1e9: below that the seven launches of the pipeline cost more than the wave kernel,
//         tools/predict_wide_probe.py).  Its epilogue reads F_x in place for D > 8192 (longer than the LDS row).
//   BIG   D > 1024: predict_big_kernel<KT>, one workgroup of 512 per (query, split); KT = 8 up to D = 4096, 16 above.
//   MFMA  B >= 256, D <= 256, predict.wave_only = 0, predict.mfma != 0: predict_mfma_kernel<NT>, NT = 2 ceil(D / 32),
//         behind row_stats_kernel (SLOT_PREDICT_STATS).
//   BULK  B >= 256, D <= 256, predict.wave_only = 0 (so predict.mfma = 0): predict_bulk_kernel<NCH>, NCH = ceil(D / 32).
//   WAVE  everything else (small batches; 256 < D <= 1024 below the work threshold; predict.wave_only = 1):
//         predict_kernel<KPL, QB>, KPL = the power of two with 64 KPL >= D, QB queries per wavefront.
// Every route but WIDE writes JS row-split partials of F_x (JS, B, D) and E (JS, B) into SLOT_PREDICT_WS; WIDE writes one
// (JS = 1).  The epilogue sums them in split order and applies J^T; with want_virial it is the one that also writes W.
#pragma once
#include <stddef.h>
#include <stdint.h>

// tile constants of the kernels (predict.hip), which the split has to respect
#define PQ 32  // predict_bulk_kernel: queries per workgroup
#define PR 32  //                      table rows per tile
#define MQ 64  // predict_mfma_kernel: queries per workgroup
#define MR 16  //                      table rows per tile

enum PredRoute { PRED_WAVE = 0, PRED_BIG = 1, PRED_BULK = 2, PRED_MFMA = 3, PRED_WIDE = 4 };

struct PredPlanIn {
  int D, N;       // D = N (N - 1) / 2
  int64_t MP, B;  // table rows, queries (both >= 1)
  int num_cus;
  bool want_virial;
  int wave_only, mfma, mfma_wide, fill;  // options predict.* (defaults 0, 1, 1, 1024)
};

struct PredPlan {
  PredRoute route;
  int sel;                       // template selector: KPL (WAVE), KT (BIG), NCH (BULK), NT (MFMA); 0 for WIDE
  int QB;                        // WAVE: queries per wavefront; 0 otherwise
  unsigned grid_x, grid_y, block;  // of the route's kernel; 0 for WIDE, whose launches predict_wide_device plans
  int JS;                        // row splits = partials the epilogue sums
  int64_t rows_per_split;
  size_t lds_bytes;              // dynamic LDS of the route's kernel
  int64_t ws_bytes;              // SLOT_PREDICT_WS: (JS, B, D) + (JS, B) doubles
  int64_t stats_bytes;           // SLOT_PREDICT_STATS: 2 MP doubles for MFMA, 0 = not requested
  bool epi_lds_row, epi_virial;  // epilogue: F_x row summed into LDS (or read in place), plain or virial
  int epi_JS;
  size_t epi_lds_bytes;
};

inline int64_t pp_ceil(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t pp_at_least_1(int64_t v) { return v > 1 ? v : 1; }

inline bool pred_route_wide(const PredPlanIn& in) {
  if (in.D > 8192) return true;  // before the options: predict.wave_only does not keep a batch off the pipeline there
  if (!(in.B >= 256 && in.D > 256 && !in.wave_only)) return false;
  // the threshold is compared in double, as the product of the three factors in this order
  return in.mfma_wide == 2 || (in.mfma_wide == 1 && (double)in.MP * (double)in.B * (double)in.D >= 1.0e9);
}

inline PredRoute pred_route(const PredPlanIn& in) {
  if (pred_route_wide(in)) return PRED_WIDE;
  if (in.D > 1024) return PRED_BIG;
  if (in.B >= 256 && in.D <= 256 && !in.wave_only) return in.mfma ? PRED_MFMA : PRED_BULK;
  return PRED_WAVE;
}

// MFMA: one workgroup per CU -- the split count (of at most 64) that minimises (rounds of workgroups) x (row tiles per
// workgroup + a fixed per-workgroup cost of ~3 tiles); the first of equals
inline int64_t pred_mfma_splits(int64_t MP, int64_t n_qt, int64_t max_js, int64_t ncu) {
  int64_t best = 1, best_cost = INT64_MAX;
  for (int64_t js = 1; js <= 64 && js <= max_js; ++js) {
    const int64_t rows = pp_ceil(pp_ceil(MP, js), MR) * MR;
    const int64_t js_eff = pp_ceil(MP, rows);
    const int64_t rounds = pp_ceil(n_qt * js_eff, ncu);
    const int64_t cost = rounds * (rows / MR + 3);
    if (cost < best_cost) {
      best_cost = cost;
      best = js;
    }
  }
  return best;
}

inline PredPlan predict_plan(const PredPlanIn& in) {
  const int D = in.D;
  const int64_t MP = in.MP, B = in.B;
  PredPlan p = {};
  p.route = pred_route(in);
  p.epi_virial = in.want_virial;
  if (p.route == PRED_WIDE) {
    p.JS = p.epi_JS = 1;
    p.rows_per_split = MP;
    p.ws_bytes = (B * (int64_t)D + B) * 8;
    p.epi_lds_row = D <= 8192;
    p.epi_lds_bytes = p.epi_lds_row ? (size_t)D * 8 : 0;
    return p;
  }
  // wanted splits = (workgroups or wavefronts that fill the chip) / (query tiles), capped so that a split keeps rows
  int64_t n_qt, JS, max_js;
  switch (p.route) {
    case PRED_BIG:
      p.sel = D <= 4096 ? 8 : 16;
      n_qt = B;
      JS = pp_ceil(1024, n_qt);
      max_js = pp_at_least_1(MP / 4);
      p.block = 512;
      break;
    case PRED_BULK:
      p.sel = (D + 31) / 32;
      n_qt = pp_ceil(B, PQ);
      JS = pp_ceil(2048, n_qt);
      max_js = pp_at_least_1(MP / 64);
      p.block = 256;
      break;
    case PRED_MFMA:
      p.sel = 2 * ((D + 31) / 32);  // even number of 16-column tiles
      n_qt = pp_ceil(B, MQ);
      max_js = pp_at_least_1(MP / 64);
      JS = pred_mfma_splits(MP, n_qt, max_js, in.num_cus);
      p.block = 256;
      p.lds_bytes = (size_t)4 * MR * (16 * p.sel + 2) * 8;  // 2 x (X tile | JA tile), pitch 16 NT + 2
      p.stats_bytes = 2 * MP * 8;
      break;
    default: {  // PRED_WAVE; the other routes never read QB, so it is worked out here only
      p.sel = 1;
      while (p.sel * 64 < D) p.sel <<= 1;
      int QB = p.sel <= 4 ? 8 : (p.sel == 8 ? 4 : (p.sel == 16 ? 2 : 1));  // what fits the registers of predict_kernel<KPL, QB>
      while (QB > 1 && B < QB) QB >>= 1;  // do not waste query slots
      // small batches: fewer queries per wavefront until the grid (query tiles x row splits) fills the chip.  The rule
      // counts with the cap of the splits (MP / 16), not with the split count chosen below: kept as it is.
      const int64_t js_cap = pp_at_least_1(MP / 16);
      while (QB > 1 && pp_ceil(B, QB) * js_cap < in.fill) QB >>= 1;
      p.QB = QB;
      n_qt = pp_ceil(B, QB);
      JS = pp_ceil(4096, n_qt);
      max_js = js_cap;
      p.block = 256;
    }
  }
  if (JS > max_js) JS = max_js;
  if (JS < 1) JS = 1;
  // rows per split (whole row tiles for BULK and MFMA: PR, a multiple of MR), then only the splits that hold rows
  int64_t rps = pp_ceil(MP, JS);
  if (p.route == PRED_BULK || p.route == PRED_MFMA) rps = pp_ceil(rps, PR) * PR;
  JS = pp_ceil(MP, rps);
  p.JS = p.epi_JS = (int)JS;
  p.rows_per_split = rps;
  if (p.route == PRED_WAVE) {  // four wavefronts per workgroup, one (query tile, split) each
    p.grid_x = (unsigned)(int)pp_ceil(n_qt * JS, 4);
    p.grid_y = 1;
  } else {
    p.grid_x = (unsigned)n_qt;
    p.grid_y = (unsigned)JS;
  }
  p.ws_bytes = (JS * B * (int64_t)D + JS * B) * 8;
  p.epi_lds_row = true;  // D <= 8192 here
  p.epi_lds_bytes = (size_t)D * 8;
  return p;
}

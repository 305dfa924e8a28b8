// Prints the factorisation's launch plan (sgdml_amd/csrc/tile_sched.h: chol_plan_build) as events for
// tests/test_chol_deep_cpu.py.  No HIP: compiled with the host compiler.
//   chol_plan_driver n n_rows NB OB outer_min_rows fused_min_rows deep deep_min_rows [summary]
// (summary: no U lines.)  The PLAN line gives the bytes of the composed launches' device tables and the longest XCD list.
// One "OP" line per operation in stream order, followed by what it does:
//   P c0 w                       panel [c0, c0 + w): diagonal block and all rows below, by the step chain
//   D c0 w                       diagonal block [c0, c0 + w) factored by workgroup 0 of this launch
//   T c0 w                       rows below the diagonal block solved
//   G r0 c0 c1 lower kb ke       C[r0:, c0:c1] -= A[r0:, kb:ke] A[c0:c1, kb:ke]^T (lower: tiles on and below the diagonal)
//   U seg ti tj kb ke counted    one 128 x 128 tile (absolute tile indices) of a composed launch
#include <cstdio>
#include <cstdlib>

#include "../sgdml_amd/csrc/tile_sched.h"

int main(int argc, char** argv) {
  if (argc != 9 && argc != 10) {
    fprintf(stderr, "usage: %s n n_rows NB OB outer_min_rows fused_min_rows deep deep_min_rows [summary]\n", argv[0]);
    return 2;
  }
  const int64_t n = atoll(argv[1]), n_rows = atoll(argv[2]);
  CholPlanOpts o;
  o.NB = atoll(argv[3]); o.OB = atoll(argv[4]); o.outer_min_rows = atoll(argv[5]); o.fused_min_rows = atoll(argv[6]);
  o.deep = atoll(argv[7]); o.deep_min_rows = atoll(argv[8]);
  const bool summary = argc == 10;
  CholPlan P;
  chol_plan_build(n, n_rows, o, &P);
  static const char* names[] = {"PANEL", "RECT", "PAIR1", "PAIR2", "FUSED", "TRSM", "TAIL", "SEG"};
  size_t words = 0, longest = 0;
  for (const PlanSegLaunch& L : P.segs) {
    words += plan_launch_words(L);
    longest = plan_launch_stride(L) > longest ? plan_launch_stride(L) : longest;
  }
  printf("PLAN NB %lld OB %lld deep %lld deep_end %lld table_bytes %zu longest_xcd_list %zu\n", (long long)P.NB, (long long)P.OB,
         (long long)P.deep, (long long)P.deep_end, words * 4, longest);
  const long long NB = P.NB, OB = P.OB, GT = 128;
  for (const CholOp& c : P.ops) {
    const long long k0 = c.k0, nb = c.nb, t0 = c.t0, nb2 = c.nb2, t1 = t0 + nb2;
    printf("OP %s %lld %lld %lld %lld\n", names[c.kind], k0, nb, t0, nb2);
    switch (c.kind) {
      case OP_PANEL: printf("P %lld %lld\n", t0, nb2); break;
      case OP_TRSM: printf("T %lld %lld\n", t0, nb2); break;
      case OP_RECT: printf("G %lld %lld %lld 0 %lld %lld\n", t0, t0, t1, k0, k0 + nb); break;
      case OP_PAIR1:
      case OP_PAIR2:
      case OP_FUSED: {
        // a list in two launches is shown as cut behind the outer panel's own columns, which the first launch must hold
        // (which launch holds which tile right of them is the balanced list's business)
        const PlanLowerLaunch& L = P.lowers[c.lower];
        const PlanSeg &u = L.upd, &s = L.second;
        const long long cut = u.origin + OB, c_lo = L.launch == 0 ? u.origin : cut, c_hi = L.launch + 1 < L.n_launch ? cut : u.origin + u.N;
        printf("G %lld %lld %lld 1 %lld %lld\n", (long long)u.origin, c_lo, c_hi, (long long)u.a_col0, (long long)(u.a_col0 + u.K));
        if (L.carries_second)
          printf("G %lld %lld %lld 1 %lld %lld\n", (long long)s.origin, (long long)s.origin, (long long)(s.origin + s.N), (long long)s.a_col0,
                 (long long)(s.a_col0 + s.K));
        printf("D %lld %lld\n", (long long)L.diag0, 64LL * L.diag_nbw);
        break;
      }
      case OP_TAIL:
        printf("P %lld %lld\n", t0, nb2);
        printf("G %lld %lld %lld 1 %lld %lld\n", t1, t1, (long long)n, k0, k0 + nb);
        break;
      case OP_SEG: {
        const PlanSegLaunch& L = P.segs[c.seg];
        int64_t tiles = 0, mx = 0, mn = 1 << 30;
        for (int x = 0; x < 8; ++x) {
          int64_t cost = 0;
          for (uint32_t v : L.xcd[x]) {
            const PlanSeg& s = L.seg[TS_SEG_ID(v)];
            const long long ti = TS_SEG_TI(v), tj = TS_SEG_TJ(v);
            if (ti * GT >= s.M || tj * GT >= s.N || s.K <= 0) { fprintf(stderr, "tile outside its segment\n"); return 1; }
            if (!summary)
              printf("U %d %lld %lld %lld %lld %u\n", TS_SEG_ID(v), s.origin / GT + ti, s.origin / GT + tj, (long long)s.a_col0,
                     (long long)(s.a_col0 + s.K), (unsigned)TS_SEG_COUNTED(v));
            cost += s.K + cp_detail::TURNOVER;
            ++tiles;
          }
          mx = cost > mx ? cost : mx;
          mn = cost < mn ? cost : mn;
        }
        if (tiles != L.tiles) { fprintf(stderr, "tile count\n"); return 1; }
        printf("D %lld %lld\n", (long long)L.diag0, NB);
        printf("S tiles %lld far %lld flops %.17g far_flops %.17g xcd_cost_min %lld xcd_cost_max %lld counted %d\n", (long long)L.tiles,
               (long long)L.far_tiles, L.flops, L.far_flops, (long long)mn, (long long)mx, L.counted);
        break;
      }
    }
  }
  return 0;
}

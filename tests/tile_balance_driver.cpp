// Stand-alone check of the tile schedule of the lower trailing updates (sgdml_amd/csrc/tile_sched.h): runs the exact
// decode the kernels use for every block index of a launch, on the CPU.  Launches are given as the plan's descriptions
// (PlanLowerLaunch) and turned into lists and ranges by the functions the launcher calls (plan_lower_sched, plan_lower_range).  Built and run by test_tile_balance_cpu.py
// (host compiler, -fsanitize=address,undefined).  Prints one line per group of cases; exit status 0 = all passed.
#include "../sgdml_amd/csrc/tile_sched.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static const int GT = 128;
static int g_fail = 0;
static long g_lists = 0;

#define CHECK(cond, ...)                                    \
  do {                                                      \
    if (!(cond)) {                                          \
      if (++g_fail <= 40) {                                 \
        std::printf("FAIL %s: ", #cond);                    \
        std::printf(__VA_ARGS__);                           \
        std::printf("\n");                                  \
      }                                                     \
    }                                                       \
  } while (0)

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// One tile list, given by the description D of any of its launches (tile_sched.h: PlanLowerLaunch): D.upd lower, in D.n_launch
// launches, the last led by the second problem D.second.  The list comes from plan_lower_sched, as in the launcher.
static void check_list(const PlanLowerLaunch& D) {
  const int tiles_m = (int)ceil_div(D.upd.M, GT), tiles_n = (int)ceil_div(D.upd.N, GT), n_launch = D.n_launch;
  const bool col0 = D.col0_first != 0;
  const int64_t M2 = D.second.M, N2 = D.second.N, K = D.upd.K, M = D.upd.M;
  const int rr = D.diag_nbw * 64 / GT;  // tile rows of the diagonal block
  ++g_lists;
  char tag[160];
  std::snprintf(tag, sizeof tag, "tiles %d x %d col0 %d launches %d second %lld x %lld", tiles_m, tiles_n, (int)col0, n_launch,
                (long long)M2, (long long)N2);
  // second problem: compact decode covers its tiles exactly once.  Its workgroup q runs lead2 - q places in front of the
  // list's block 0 (gemm_block: blocks below tiles2 are the second problem's), i.e. on the XCD labelled (q - lead2) mod 8.
  double base[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (M2 > 0) {
    const int tm2 = (int)ceil_div(M2, GT), tn2 = (int)ceil_div(N2, GT);
    bool compact = false;
    const int lead2 = plan_second_blocks(M2, N2, &compact);
    CHECK(compact && tm2 >= tn2, "%s", tag);
    std::vector<int> seen2((size_t)tm2 * tn2, 0);
    for (int q = 0; q < lead2; ++q) {
      int64_t ti, tj;
      tile_decode_second(q, tn2, &ti, &tj);
      CHECK(ti >= 0 && ti < tm2 && tj >= 0 && tj < tn2 && !(ti < tn2 && tj > ti), "%s second q %d -> %lld %lld", tag, q, (long long)ti, (long long)tj);
      if (ti >= 0 && ti < tm2 && tj >= 0 && tj < tn2) ++seen2[(size_t)ti * tn2 + tj];
      base[((q - lead2) % 8 + 8) % 8] += (double)D.second.K / (double)K;
    }
    for (int i = 0; i < tm2; ++i)
      for (int j = 0; j < tn2; ++j) CHECK(seen2[(size_t)i * tn2 + j] == ((i < tn2 && j > i) ? 0 : 1), "%s second tile %d %d", tag, i, j);
  }
  TileSched S;
  plan_lower_sched(D, &S);
  CHECK(S.ok, "%s: no schedule", tag);
  if (!S.ok) return;
  for (int x = 0; x < 8; ++x) CHECK(S.base_last[x] == base[x], "%s XCD %d: dealt around %.2f, the second problem puts %.2f there", tag, x, S.base_last[x], base[x]);
  std::vector<int> seen((size_t)tiles_m * tiles_m, 0), where((size_t)tiles_m * tiles_m, -1);
  const double rl = (double)(M - (int64_t)(tiles_m - 1) * GT);
  double flops_sum = 0.0;
  for (int l = 0; l < n_launch; ++l) {
    TileLaunch L = S.L[l];
    L.table = S.table[l].data();
    CHECK(S.blocks[l] % 8 == 0, "%s", tag);
    CHECK((int64_t)S.table[l].size() == 8 * (int64_t)L.stride, "%s", tag);
    double work[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tile_flops = 0.0;
    int64_t empty = 0, counted = 0, held = 0;
    bool past_col0[8] = {};
    for (int64_t b = 0; b < S.blocks[l]; ++b) {
      int64_t ti = -1, tj = -1;
      if (!tile_decode_bal(L, b, &ti, &tj)) { ++empty; continue; }
      const bool in = ti >= 0 && ti < tiles_m && tj >= 0 && tj < tiles_n && tj <= ti;
      CHECK(in, "%s launch %d block %lld -> tile %lld %lld", tag, l, (long long)b, (long long)ti, (long long)tj);
      if (!in) continue;
      ++held;
      ++seen[(size_t)ti * tiles_m + tj];
      where[(size_t)ti * tiles_m + tj] = l;
      work[b & 7] += 1.0;
      if (ti < rr && tj < rr) ++counted;
      if (col0) {  // on every XCD the first-column tiles come before all others
        if (tj >= 8) past_col0[b & 7] = true;
        else CHECK(!past_col0[b & 7] && l == 0, "%s launch %d block %lld: first-column tile %lld %lld behind others", tag, l, (long long)b, (long long)ti, (long long)tj);
      }
      const double rows = (ti == tiles_m - 1) ? rl : (double)GT;
      tile_flops += (ti == tj) ? rows * (rows + 1.0) * (double)K : 2.0 * rows * (double)GT * (double)K;
    }
    CHECK(held == S.tiles[l], "%s launch %d: %lld tiles decoded, %lld counted by the scheduler", tag, l, (long long)held, (long long)S.tiles[l]);
    CHECK(empty < 8, "%s launch %d: %lld empty blocks", tag, l, (long long)empty);
    if (col0) {
      int want = 0;  // the lower tiles of the leading tile block: the diagonal block's (10 at NB = 512)
      for (int i = 0; i < rr && i < tiles_m && l == 0; ++i)
        for (int j = 0; j <= i && j < tiles_n; ++j) ++want;
      CHECK(counted == want, "%s launch %d: %lld counted tiles", tag, l, (long long)counted);
    }
    // balance: work per XCD (tiles; the second problem's at K2 / K) within one tile row of the launch's mean
    double mean = 0.0;
    for (int x = 0; x < 8; ++x) {
      if (l == n_launch - 1) work[x] += base[x];
      mean += work[x] / 8.0;
    }
    for (int x = 0; x < 8; ++x) CHECK(std::fabs(work[x] - mean) < 8.0, "%s launch %d XCD %d: work %.1f, mean %.2f", tag, l, x, work[x], mean);
    const double fl = tile_sched_flops(S, l, M, K, tiles_m, GT);
    if (l < n_launch - 1 || tiles_n == tiles_m) CHECK(fl == tile_flops, "%s launch %d: flops %.0f, tiles %.0f", tag, l, fl, tile_flops);
    else CHECK(fl == tile_flops + rl * (rl + 1.0) * (double)K, "%s launch %d: flops %.0f, tiles %.0f", tag, l, fl, tile_flops);
    flops_sum += fl;
  }
  CHECK(flops_sum == (double)M * (double)(M + 1) * (double)K, "%s: flops of the list %.0f", tag, flops_sum);
  for (int i = 0; i < tiles_m; ++i)
    for (int j = 0; j < tiles_m; ++j) {
      const int want = (j <= i && j < tiles_n) ? 1 : 0;
      CHECK(seen[(size_t)i * tiles_m + j] == want, "%s: tile %d %d produced %d times", tag, i, j, seen[(size_t)i * tiles_m + j]);
      if (want && col0 && j < 8) CHECK(where[(size_t)i * tiles_m + j] == 0, "%s: first-column tile %d %d in launch %d", tag, i, j, where[(size_t)i * tiles_m + j]);
    }
  if (n_launch == 2) {  // the cut: about half the tiles, the first launch whole rounds behind the head
    const int64_t all = S.tiles[0] + S.tiles[1];
    const int64_t rounds = S.L[1].r1;
    if (rounds >= 4) CHECK(std::llabs(2 * S.tiles[0] - all) <= 512 + 2 * 8 * (int64_t)tiles_m, "%s: first launch %lld of %lld tiles", tag, (long long)S.tiles[0], (long long)all);
    CHECK(ts_unpack(S.L[0].tn, 0) == 0 && S.L[0].r1 == S.L[1].r0 && S.L[0].r0 == 0, "%s: cut", tag);
  }
}

// the super-tile enumeration (gemm.balance = 0) against a restatement with explicit loops
static void check_super(int tiles_m, int tiles_n, bool col0, int64_t s_begin, int64_t n_super) {
  const int sm = (tiles_m + 7) / 8;
  std::vector<std::pair<int, int>> order;
  if (col0) {
    for (int SI = 0; SI < sm; ++SI) order.push_back({SI, 0});
    for (int SI = 1; SI < sm; ++SI)
      for (int SJ = 1; SJ <= SI; ++SJ) order.push_back({SI, SJ});
  } else {
    for (int SI = 0; SI < sm; ++SI)
      for (int SJ = 0; SJ <= SI; ++SJ) order.push_back({SI, SJ});
  }
  const int64_t n_all = (int64_t)sm * (sm + 1) / 2;
  CHECK((int64_t)order.size() == n_all, "super list");
  CHECK(0 <= s_begin && n_super <= n_all, "super range");
  if (n_super <= s_begin) return;
  const int64_t blocks = (n_super - s_begin + 7) / 8 * 512;
  std::vector<int64_t> want_ti((size_t)blocks, -1), want_tj((size_t)blocks, -1);
  for (int64_t s = s_begin; s < n_super; ++s)
    for (int r = 0; r < 8; ++r)
      for (int c = 0; c < 8; ++c) {
        const int64_t rel = s - s_begin, b = (((rel / 8) * 64 + r * 8 + c) << 3) + rel % 8;
        const int64_t ti = order[(size_t)s].first * 8 + r, tj = order[(size_t)s].second * 8 + c;
        if (ti < tiles_m && tj < tiles_n && tj <= ti) { want_ti[(size_t)b] = ti; want_tj[(size_t)b] = tj; }
      }
  for (int64_t b = 0; b < blocks; ++b) {
    int64_t ti = -1, tj = -1;
    const bool has = tile_decode_super(b, 1, col0 ? 1 : 0, tiles_m, tiles_n, (tiles_n + 7) / 8, s_begin, n_super, &ti, &tj);
    if (!has) ti = tj = -1;
    CHECK(ti == want_ti[(size_t)b] && tj == want_tj[(size_t)b], "super enumeration tiles %d x %d col0 %d block %lld: %lld %lld, expected %lld %lld", tiles_m,
          tiles_n, (int)col0, (long long)b, (long long)ti, (long long)tj, (long long)want_ti[(size_t)b], (long long)want_tj[(size_t)b]);
  }
}

// plan_lower_range against the expression it replaced: launches took a share (f0, f1) of the super-tile list, and a list
// in two launches was cut at fs = (s_split + 0.5) / n_all
static void check_range(int tiles_m) {
  const int64_t sm = (tiles_m + 7) / 8, n_all = sm * (sm + 1) / 2;
  int64_t s_split = n_all / 2;
  if (s_split < sm) s_split = sm;
  const double fs = ((double)s_split + 0.5) / (double)n_all;
  const double f[3][2] = {{0.0, 1.0}, {0.0, fs}, {fs, 1.0}};  // the only launch, the first of two, the second of two
  for (int i = 0; i < 3; ++i) {
    PlanLowerLaunch D = plan_lower_plain((int64_t)tiles_m * GT, (int64_t)tiles_m * GT, 512);
    D.n_launch = i == 0 ? 1 : 2; D.launch = i == 2 ? 1 : 0;
    int64_t s0, s1;
    plan_lower_range(D, &s0, &s1);
    const int64_t s_begin = (int64_t)(f[i][0] * (double)n_all), n_super = (f[i][1] >= 1.0) ? n_all : (int64_t)(f[i][1] * (double)n_all);
    CHECK(s0 == s_begin && s1 == (n_super < s_begin ? s_begin : n_super), "range tiles_m %d launch %d of %d: [%lld, %lld), expected [%lld, %lld)",
          tiles_m, D.launch, D.n_launch, (long long)s0, (long long)s1, (long long)s_begin, (long long)n_super);
  }
}

// every lower launch of the factorisation's plan with the one-level schedule (chol.deep = 0): the fused launches from their
// descriptions, the tail's plain lower update as chol_factor_device hands it to launch_gemm_nt_sub
static void check_factorisation(int64_t n, int64_t n_rows, CholPlanOpts o = CholPlanOpts()) {
  o.deep = 0;
  CholPlan P;
  chol_plan_build(n, n_rows, o, &P);
  long pairs = 0, singles = 0, plain = 0;
  int ready = 0;  // counted tiles so far
  std::array<int64_t, 7> first_key = {};
  auto check_launch = [&](const PlanLowerLaunch& D) {
    if (D.launch == 0) check_list(D);
    if (D.launch == 0) first_key = plan_lower_key(D);
    CHECK(plan_lower_key(D) == first_key, "n %lld: the two launches of a list describe different lists", (long long)n);
    int64_t s_begin, n_super;
    plan_lower_range(D, &s_begin, &n_super);
    check_super((int)ceil_div(D.upd.M, GT), (int)ceil_div(D.upd.N, GT), D.col0_first != 0, s_begin, n_super);
  };
  for (const CholOp& c : P.ops) {
    if (c.lower >= 0) {
      const PlanLowerLaunch& D = P.lowers[(size_t)c.lower];
      CHECK(D.upd.M > 0 && D.upd.N > 0 && D.upd.K > 0 && D.diag_nbw > 0, "n %lld: empty fused launch", (long long)n);
      check_launch(D);
      CHECK(c.ready_target == (D.counted ? (ready += D.counted) : 0), "n %lld: tile counter target %d", (long long)n, c.ready_target);
      if (c.kind == OP_PAIR1) ++pairs;
      if (c.kind == OP_FUSED) ++singles;
    } else if (c.kind == OP_TAIL) {
      const int64_t t1 = c.t0 + c.nb2;
      check_launch(plan_lower_plain(n_rows - t1, n - t1, c.nb));
      ++plain;
    }
  }
  std::printf("factorisation n %lld rows %lld: %ld pairs, %ld single fused, %ld plain lower launches (chol.nb = %lld)\n", (long long)n,
              (long long)n_rows, pairs, singles, plain, (long long)P.NB);
}

int main() {
  std::vector<int> sizes;
  for (int t = 1; t <= 40; ++t) sizes.push_back(t);
  sizes.push_back(320);
  sizes.push_back(481);
  for (int tm : sizes)
    for (int dn = 0; dn < 2; ++dn) {  // with and without a carried row that opens a last tile row of its own
      const int tn = tm - dn;
      if (tn < 1) continue;
      const int64_t Ms[3] = {(int64_t)(tm - 1) * GT + 1, (int64_t)(tm - 1) * GT + 77, (int64_t)tm * GT};
      for (int64_t M : Ms) {
        if (dn == 1 && M != Ms[0]) continue;
        for (int col0 = 0; col0 < 2; ++col0)
          for (int nl = 1; nl <= 2; ++nl) {
            PlanLowerLaunch D = plan_lower_plain(M, M - dn, 1024);
            D.col0_first = col0; D.n_launch = nl; D.diag_nbw = 8;
            check_list(D);
            if (tm >= 8) {  // second problem: the rows below the first four tile rows, four tile columns, half and full depth
              D.second.M = M - 4 * GT; D.second.N = 4 * GT; D.second.K = 512;
              check_list(D);
              D.upd.K = 512;
              check_list(D);
            }
          }
      }
      const int64_t n_all = (int64_t)((tm + 7) / 8) * ((tm + 7) / 8 + 1) / 2;
      for (int col0 = 0; col0 < 2; ++col0) {  // the whole list and its halves
        check_super(tm, tn, col0 != 0, 0, n_all);
        check_super(tm, tn, col0 != 0, 0, n_all / 2);
        check_super(tm, tn, col0 != 0, n_all / 2, n_all);
      }
      if (dn == 0) check_range(tm);
    }
  std::printf("shapes: %ld lists\n", g_lists);
  check_factorisation(63000, 63001);
  check_factorisation(2500, 2501);
  // chol.nb = 128 with the thresholds of tests/test_tile_balance_gpu.py: the small-panel pair, fused and tail arms
  for (int i = 0; i < 2; ++i) {
    CholPlanOpts o;
    o.NB = 128; o.OB = 256; o.outer_min_rows = i ? 2000 : 1500; o.fused_min_rows = i ? 1000 : 700;
    check_factorisation(63000, 63001, o);
    check_factorisation(2500, 2501, o);
  }
  std::printf("%ld lists checked, %d failures\n", g_lists, g_fail);
  return g_fail ? 1 : 0;
}

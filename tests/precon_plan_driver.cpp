// Stand-alone printer of the Nystroem / preconditioner plans (sgdml_amd/csrc/precon_plan.h).  Built and run by
// test_precon_plan_cpu.py (host compiler, -fsanitize=address,undefined).  Reads one request per line from standard input,
//   gram  n m ldc split_option
//   form  option chunk m
//   chunk option n_loc
//   apply form n_loc m ld gemv_plain f32_rows_per f32_rw
// and prints one line per request: the request, " : ", then every field of the plan as "name value" pairs.
#include "../sgdml_amd/csrc/precon_plan.h"

#include <cstdio>
#include <cstring>

int main() {
  char kind[16];
  long long a[7];
  while (std::scanf("%15s", kind) == 1) {
    if (!std::strcmp(kind, "gram")) {
      if (std::scanf("%lld %lld %lld %lld", a, a + 1, a + 2, a + 3) != 4) return 1;
      const GramSplitPlan p = gram_split_plan(a[0], a[1], a[2], (int)a[3]);
      std::printf("gram %lld %lld %lld %lld : tiles %d T %lld S %d rows_per %lld part_bytes %lld\n", a[0], a[1], a[2], a[3], p.tiles,
                  (long long)p.T, p.S, (long long)p.rows_per, (long long)p.part_bytes);
    } else if (!std::strcmp(kind, "form")) {
      if (std::scanf("%lld %lld %lld", a, a + 1, a + 2) != 3) return 1;
      std::printf("form %lld %lld %lld : form %d\n", a[0], a[1], a[2], choose_precon_form((int)a[0], a[1], a[2]));
    } else if (!std::strcmp(kind, "chunk")) {
      if (std::scanf("%lld %lld", a, a + 1) != 2) return 1;
      std::printf("chunk %lld %lld : chunk %lld\n", a[0], a[1], (long long)f32_gram_chunk(a[0], a[1]));
    } else if (!std::strcmp(kind, "apply")) {
      if (std::scanf("%lld %lld %lld %lld %lld %lld %lld", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6) != 7) return 1;
      const PreconOpts o = {(int)a[4], (int)a[5], (int)a[6]};
      const PreconApplyPlan p = precon_apply_plan((int)a[0], a[1], a[2], a[3], o);
      std::printf("apply %lld %lld %lld %lld %lld %lld %lld : form %d nt %d rows_per %d nparts %d rw %d col_blocks %u row_blocks %u "
                  "o_t %lld o_u %lld n_u %lld ws_bytes %lld launches %d work %.17g\n",
                  a[0], a[1], a[2], a[3], a[4], a[5], a[6], p.form, (int)p.nt, p.rows_per, p.nparts, p.rw, p.col_blocks, p.row_blocks,
                  (long long)p.o_t, (long long)p.o_u, (long long)p.n_u, (long long)p.ws_bytes, p.launches, p.work);
    } else {
      return 1;
    }
  }
  return 0;
}

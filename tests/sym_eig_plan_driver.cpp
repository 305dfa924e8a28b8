// Stand-alone printer of the eigensolver's plan, the slice length and the slice workspace (sgdml_amd/csrc/sym_eig_plan.h).
// Built and run by test_sym_eig_plan_cpu.py (host compiler, -fsanitize=address,undefined).  Reads one request per line from
// standard input,
//   plan  num_cus M N cap_global
//   slice num_cus B n3 option
//   ws    len N work_doubles with_R
// and prints one line per request: the request, " : ", then every field as "name value" pairs.
#include "../sgdml_amd/csrc/sym_eig_plan.h"

#include <cstdio>
#include <cstring>

int main() {
  char kind[16];
  long long a[4];
  while (std::scanf("%15s %lld %lld %lld %lld", kind, a, a + 1, a + 2, a + 3) == 5) {
    std::printf("%s %lld %lld %lld %lld : ", kind, a[0], a[1], a[2], a[3]);
    if (!std::strcmp(kind, "plan")) {
      const SymEigPlan p = sym_eig_plan((int)a[0], a[1], (int)a[2], a[3] != 0);
      std::printf("NP %d a_in_lds %d v_in_lds %d lds %lld grid %lld work_doubles %lld\n", p.NP, p.a_in_lds, p.v_in_lds,
                  (long long)p.lds, (long long)p.grid, (long long)p.work_doubles);
    } else if (!std::strcmp(kind, "slice")) {
      std::printf("len %lld\n", (long long)spectrum_slice_len((int)a[0], a[1], (int)a[2], a[3]));
    } else if (!std::strcmp(kind, "ws")) {
      const SpectrumWs s = spectrum_ws(a[0], (int)a[1], a[2], a[3] != 0);
      std::printf("work %lld H %lld R %lld F %lld w %lld info %lld E %lld mass %lld sweeps %lld n_rigid %lld n_neg %lld with_R %d "
                  "per_geometry %lld total %lld\n",
                  (long long)s.work, (long long)s.H, (long long)s.R, (long long)s.F, (long long)s.w, (long long)s.info,
                  (long long)s.E, (long long)s.mass, (long long)s.sweeps, (long long)s.n_rigid, (long long)s.n_neg, s.with_R,
                  (long long)s.per_geometry, (long long)s.total);
    } else {
      return 1;
    }
  }
  return 0;
}

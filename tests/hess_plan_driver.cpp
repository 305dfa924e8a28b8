// Stand-alone printer of the analytic Hessian's plan (sgdml_amd/csrc/hess_plan.h).  Built and run by test_hess_plan_cpu.py
// (host compiler, -fsanitize=address,undefined).  Reads one input per line from standard input,
//   N MP B generic chunk_rows
// and prints one line per input: the input, every field of the plan, then per row chunk "nr,groups,grid_x,rps,accumulate" and
// per batch slice bs.  An unsupported size prints "supported 0" and nothing else.
#include "../sgdml_amd/csrc/hess_plan.h"

#include <cstdio>

int main() {
  long long N, MP, B, generic, chunk_rows;
  while (std::scanf("%lld %lld %lld %lld %lld", &N, &MP, &B, &generic, &chunk_rows) == 5) {
    HessPlanIn in;
    in.N = (int)N;
    in.MP = MP;
    in.B = B;
    in.generic = (int)generic;
    in.chunk_rows = chunk_rows;
    const HessPlan p = hess_plan(in);
    std::printf("%lld %lld %lld %lld %lld : supported %d", N, MP, B, generic, chunk_rows, (int)p.supported);
    if (p.supported) {
      std::printf(" variant %s sel %d v_lds %d lds %zu D %d n3 %d nb %d ld %d n_tp %d Bs %lld RG %d nr_cap %lld G %lld JS %lld "
                  "nU %lld nCS %lld nPF %lld nPE %lld nHp %lld nFX %lld nTau %lld ws %lld",
                  p.variant == HESS_WAVE ? "wave" : "block", p.sel, p.v_lds, p.lds_bytes, p.D, p.n3, p.nb, p.ld, p.n_tp,
                  (long long)p.Bs, p.RG, (long long)p.nr_cap, (long long)p.G, (long long)p.JS, (long long)p.nU, (long long)p.nCS,
                  (long long)p.nPF, (long long)p.nPE, (long long)p.nHp, (long long)p.nFX, (long long)p.nTau, (long long)p.ws_bytes);
      std::printf(" oW %lld oCS %lld oPF %lld oPE %lld oHp %lld oFX %lld oTau %lld", (long long)p.oW, (long long)p.oCS, (long long)p.oPF,
                  (long long)p.oPE, (long long)p.oHp, (long long)p.oFX, (long long)p.oTau);
      std::printf(" chunks");
      for (int64_t r0 = 0; r0 < MP; r0 += p.nr_cap) {
        const HessChunk c = p.chunk(r0);
        std::printf(" %lld,%lld,%u,%lld,%d", (long long)c.nr, (long long)c.groups, c.grid_x, (long long)c.rps, c.accumulate);
      }
      std::printf(" slices");
      for (int64_t b0 = 0; b0 < B; b0 += p.Bs) std::printf(" %d", p.slice(b0));
    }
    std::printf("\n");
  }
  return 0;
}

"""A/B of factorisation options at the benchmark size: python tools/chol_ab.py "key=val,key=val" "key=val" ...
(each argument = one option set; '-' = defaults).  Prints factor time (3 repetitions) and the solve residual.

  --alternate N   ONE context, the option sets taken in turn N times (A B A B ...): what a schedule option such as
                  chol.deep = 0 against the default has to be judged by -- the gain counts
                  against the max - min spread of the first set's runs in the same process.  An option cannot be put
                  back to the library's default once set, so every set must name the same options (chol.deep=0 against
                  chol.deep=4096, not against '-').  After the timed runs each set is run once more under the per-kernel
                  timers: fused trailing-update launches, their time, their rate, and the far tiles' share of the flops.
"""
import sys, os
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from bench import synth_geometries
from sgdml_amd import _lib

M, N = int(os.environ.get('AB_M', '1000')), 21
R, E, F = synth_geometries(N, M, seed=0)
tp = np.arange(N * (N - 1) // 2, dtype=np.int64)[None]
y = F.ravel() / np.std(F)


def parse(spec):
    return {} if spec == '-' else {k: float(v) for k, v in (kv.split('=') for kv in spec.split(','))}


def factor_once(ctx):
    ctx.assemble_K(20.0, False, alloc_extra_rows=1, for_cholesky=1e-10)
    ctx.chol_set_rhs(y)
    info = ctx.chol_factor(1e-10)
    return ctx.phase_ms('factor')[0], info


def residual(ctx, xd):
    a = ctx.chol_solve(None)
    ctx.predict_upload_model(xd, np.zeros_like(xd), tp, 20.0, None)
    Kv = ctx.kernel_matvec(1e-10, False, -a)
    return np.linalg.norm(-Kv - y) / np.linalg.norm(y)


args = sys.argv[1:]
if args and args[0] == '--alternate':
    reps, specs = int(args[1]), args[2:]
    if len({tuple(sorted(parse(s))) for s in specs}) != 1:
        sys.exit('--alternate: every option set must name the same options')
    ctx = _lib.Context(0)
    xd, gd = ctx.desc_from_R(R.reshape(M, -1), N)
    ctx.train_upload(xd, gd, tp)

    def select(spec):
        for k, v in parse(spec).items():
            ctx.set_option(k, v)

    select(specs[0])
    factor_once(ctx)  # the process's first factorisation (allocation, code objects, launch tables) is not a sample
    times = {s: [] for s in specs}
    for rep in range(reps):
        for s in specs:
            select(s)
            factor_once(ctx)  # the first run after a switch builds or re-reads the set's launch tables
            times[s].append(factor_once(ctx)[0])
    base = times[specs[0]]
    print('%-46s %s   mean %.1f  spread %.1f ms' % (specs[0], ' '.join('%.1f' % t for t in base), np.mean(base), max(base) - min(base)), flush=True)
    for s in specs[1:]:
        t = times[s]
        d = np.mean(base) - np.mean(t)
        print('%-46s %s   mean %.1f  spread %.1f ms   gain %.1f ms = %.1f x the spread of %s' % (
            s, ' '.join('%.1f' % v for v in t), np.mean(t), max(t) - min(t), d, d / max(max(base) - min(base), 1e-9), specs[0]), flush=True)
    for s in specs:
        select(s)
        ctx.profile(True)
        factor_once(ctx)
        ms, nl, fl = ctx.kernel_stat('gemm_nt_sub_diag')
        _, nd, fd = ctx.kernel_stat('gemm_nt_sub_deep')
        ts_ms, ts_n, _ = ctx.kernel_stat('panel_trsm')
        ctx.profile(False)
        print('%-46s fused launches %d: %.1f ms, %.2f TFLOP/s; far tiles in %d of them, %.3f of their flops; panel_trsm %d: %.1f ms; '
              'resid %.2e' % (s, nl, ms, fl / ms * 1e-9 if ms else 0.0, nd, fd / fl if fl else 0.0, ts_n, ts_ms, residual(ctx, xd)), flush=True)
    ctx.close()
    sys.exit(0)

for spec in (args or ['-']):
    ctx = _lib.Context(0)
    xd, gd = ctx.desc_from_R(R.reshape(M, -1), N)
    ctx.train_upload(xd, gd, tp)
    for k, v in parse(spec).items():
        ctx.set_option(k, v)
    ts, ta = [], []
    for rep in range(3):
        t, info = factor_once(ctx)
        ta.append(ctx.phase_ms('assemble')[0])
        ts.append(t)
    res = residual(ctx, xd)
    print('%-40s factor %s ms  info %d  resid %.2e  assemble %s ms' % (spec, ' '.join('%.1f' % t for t in ts), info, res,
                                                                            ' '.join('%.2f' % t for t in ta)), flush=True)
    ctx.close()

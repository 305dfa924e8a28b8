"""Per-launch model of how the tiles of the Cholesky's trailing updates fall on the 8 XCDs, next to measured launch times.

  python tools/xcd_balance_model.py [n] [n_rows] [trace_balance0.csv trace_balance1.csv]

Restates the launch sequence of chol_factor_device (csrc/chol.hip, default options) and the super-tile enumeration of
tile_decode_super (csrc/tile_sched.h): block b runs on XCD b % 8 (round-robin dealing, MI355X_MICROARCH "Workgroup
dispatch"), an XCD has 64 workgroup slots, a launch ends when its most loaded XCD ends.  Per launch: tiles, rounds
(tiles / 512), the most loaded XCD's excess over the mean in rounds, and the time that excess would cost at the tile time of
the launch's depth (225 us at K = 1024).  With two rocprofv3 kernel-trace CSVs (one factorisation or more per file; the last
one is taken) the measured duration of each launch under gemm.balance = 0 and 1 is printed beside the prediction.

  python tools/xcd_balance_model.py --deep DRIVER [n] [n_rows] [W] [deep_min_rows] [trace.csv]

models the COMPOSED launches of the deep schedule (chol.deep = W), whose near tiles (K = 1024 / 512) and far tiles (K = W) differ
in length: DRIVER is tests/chol_plan_driver.cpp compiled with the host compiler; it prints the plan chol_factor_device runs.
A tile costs K + 66 in units of k (66 = tile turnover, fitted to 0.885 of the peak at K = 1024 and 0.927 at K = 4096); this is
the cost chol_plan_build sizes the launches' shares and deals the XCDs by.  Per launch: tiles, far tiles, the most and least
loaded XCD, the predicted time (most loaded XCD / 64 slots) and, with a kernel-trace CSV, the measured duration and rate."""
import csv
import subprocess
import sys

GT, TILE_US_K1024 = 128, 225.0


def cdiv(a, b):
    return -(-a // b)


def launches(n, n_rows, NB=512, OB=1024, min_rows=12288, outer_min_rows=16384):
    """(kernel, M, N, K, lower, col0_first, f0, f1, second (M2, N2, K2) or None) in launch order."""
    def width_at(c0):
        left = n - (c0 + OB)
        return min(OB if (left > 0 and left >= outer_min_rows) else NB, n - c0)

    out = []
    k0, nb = 0, min(n, NB)
    while True:
        t0 = k0 + nb
        if t0 >= n:
            break
        nb2 = width_at(t0)
        t1 = t0 + nb2
        fuse = nb2 % 64 == 0 and n - t1 >= min_rows and n_rows - t1 > 0
        if fuse and nb2 == 2 * NB:
            ta = t0 + NB
            sm = cdiv(cdiv(n_rows - t0, GT), 8)
            n_all = sm * (sm + 1) // 2
            fs = (max(n_all // 2, sm) + 0.5) / n_all
            out.append(('diag', n_rows - t0, n - t0, nb, 1, 1, 0.0, fs, None))
            out.append(('diag', n_rows - t0, n - t0, nb, 1, 1, fs, 1.0, (n_rows - ta, NB, NB)))
        else:
            out.append(('plain', n_rows - t0, nb2, nb, 0, 0, 0.0, 1.0, None))
            if fuse:
                out.append(('diag', n_rows - t1, n - t1, nb, 1, 0, 0.0, 1.0, None))
            elif t1 < n:
                out.append(('plain', n_rows - t1, n - t1, nb, 1, 0, 0.0, 1.0, None))
        k0, nb = t0, nb2
    return out


def xcd_work(kernel, M, N, K, lower, col0, f0, f1, second):
    """Tiles per XCD (second problem's at K2 / K) under the super-tile enumeration."""
    tm, tn = cdiv(M, GT), cdiv(N, GT)
    sm, sn = cdiv(tm, 8), cdiv(tn, 8)
    if lower:
        order = ([(i, 0) for i in range(sm)] + [(i, j) for i in range(1, sm) for j in range(1, i + 1)]) if col0 else \
                [(i, j) for i in range(sm) for j in range(i + 1)]
    else:
        order = [(i, j) for i in range(sm) for j in range(sn)]
    n_all = len(order)
    s0, s1 = int(f0 * n_all), (n_all if f1 >= 1.0 else int(f1 * n_all))
    work = [0.0] * 8
    lead = 1 if kernel == 'diag' else 0
    if second:
        M2, N2, K2 = second
        tm2, tn2 = cdiv(M2, GT), cdiv(N2, GT)
        for q in range(tm2 * tn2):
            i, j = divmod(q, tn2)
            if not (i < tn2 and j > i):
                work[(q + lead) % 8] += K2 / K
        lead += tm2 * tn2
    for s in range(s0, s1):
        SI, SJ = order[s]
        cnt = sum(1 for r in range(8) for c in range(8)
                  if SI * 8 + r < tm and SJ * 8 + c < tn and (not lower or SJ * 8 + c <= SI * 8 + r))
        work[(s - s0 + lead) % 8] += cnt
    return work


def read_trace(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get('Kernel_Name') or r.get('kernel_name') or ''
            kind = 'diag' if 'gemm_nt_sub_diag_kernel' in name else ('plain' if 'gemm_nt_sub_kernel' in name else None)
            if kind:
                b, e = int(r.get('Start_Timestamp') or r['start_timestamp']), int(r.get('End_Timestamp') or r['end_timestamp'])
                rows.append((b, kind, (e - b) * 1e-3))
    rows.sort()
    return rows


def last_factorisation(rows, seq):
    """Durations (us) of the launches of the last factorisation in `rows`, matched to seq by kernel kind and order."""
    n_diag = sum(1 for s in seq if s[0] == 'diag')
    diag = [r for r in rows if r[1] == 'diag'][-n_diag:]
    t_first = diag[0][0]
    it = iter([r for r in rows if r[0] >= t_first])
    out = []
    for s in seq:
        for r in it:
            if r[1] == s[0]:
                out.append(r[2])
                break
    return out


def deep_main(args):
    exe = args[0]
    n = int(args[1]) if len(args) > 1 else 63000
    n_rows = int(args[2]) if len(args) > 2 else n + 1
    W = int(args[3]) if len(args) > 3 else 4096
    deep_min = int(args[4]) if len(args) > 4 else 26624
    out = subprocess.run([exe] + [str(v) for v in (n, n_rows, 512, 1024, 16384, 12288, W, deep_min)], capture_output=True, text=True,
                         check=True).stdout
    S = []
    for ln in out.split('\n'):
        f = ln.split()
        if f and f[0] == 'S':
            S.append({f[i]: float(f[i + 1]) for i in range(1, len(f), 2)})
    meas = []
    if len(args) > 5:
        with open(args[5]) as f:
            rows = sorted((int(r['Start_Timestamp']), (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-6)
                          for r in csv.DictReader(f) if 'gemm_nt_sub_seg_kernel' in r['Kernel_Name'])
        meas = [d for _, d in rows][-len(S):]
    us_per_k = TILE_US_K1024 / (1024 + 66)
    print('# n = %d, rows = %d, chol.deep = %d, chol.deep_min_rows = %d: %d composed launches' % (n, n_rows, W, deep_min, len(S)))
    print('# %3s %7s %7s %9s %9s %8s %8s' % ('i', 'tiles', 'far', 'xcd_max', 'xcd_min', 'TFLOP', 'pred_ms') + (' %8s %7s' % ('meas_ms', 'TF/s') if meas else ''))
    tp = tm = tf = 0.0
    for i, s in enumerate(S):
        pred = s['xcd_cost_max'] / 64.0 * us_per_k * 1e-3
        line = '  %3d %7d %7d %9d %9d %8.4f %8.2f' % (i, s['tiles'], s['far'], s['xcd_cost_max'], s['xcd_cost_min'], s['flops'] * 1e-12, pred)
        tp += pred
        tf += s['flops']
        if meas:
            line += ' %8.2f %7.2f' % (meas[i], s['flops'] / meas[i] * 1e-9)
            tm += meas[i]
        print(line)
    print('# predicted %.1f ms' % tp + ('; measured %.1f ms, %.2f TFLOP/s over the composed launches' % (tm, tf / tm * 1e-9) if meas else ''))


def main():
    args = sys.argv[1:]
    if args and args[0] == '--deep':
        return deep_main(args[1:])
    n = int(args[0]) if args else 63000
    n_rows = int(args[1]) if len(args) > 1 else n + 1
    seq = launches(n, n_rows)
    meas = [last_factorisation(read_trace(p), seq) for p in args[2:4]]
    print('# n = %d, rows = %d; kernel: diag = gemm_nt_sub_diag_kernel, plain = gemm_nt_sub_kernel' % (n, n_rows))
    print('# %3s %-5s %5s %5s %5s %8s %7s %7s %9s' % ('i', 'kern', 'low', 'M/GT', 'K', 'tiles', 'rounds', 'excess', 'pred_us') +
          (' %10s %10s %9s' % ('bal0_us', 'bal1_us', 'diff_us') if len(meas) == 2 else ''))
    tot = {'diag': [0.0, 0.0, 0.0, 0.0], 'plain_lower': [0.0, 0.0, 0.0, 0.0]}
    for i, s in enumerate(seq):
        w = xcd_work(*s)
        mean = sum(w) / 8.0
        excess = (max(w) - mean) / 64.0
        pred = excess * TILE_US_K1024 * s[3] / 1024.0 if s[4] else 0.0
        line = '  %3d %-5s %5d %5d %5d %8.1f %7.2f %7.2f %9.1f' % (i, s[0], s[4], cdiv(s[1], GT), s[3], sum(w), mean / 64.0, excess, pred)
        if len(meas) == 2 and i < len(meas[0]) and i < len(meas[1]):
            line += ' %10.1f %10.1f %9.1f' % (meas[0][i], meas[1][i], meas[0][i] - meas[1][i])
            key = 'diag' if s[0] == 'diag' else ('plain_lower' if s[4] else None)
            if key:
                t = tot[key]
                t[0] += pred; t[1] += meas[0][i]; t[2] += meas[1][i]; t[3] += 1
        elif s[4]:
            key = 'diag' if s[0] == 'diag' else 'plain_lower'
            tot[key][0] += pred; tot[key][3] += 1
        print(line)
    for k, t in tot.items():
        print('# %-11s %3d launches: predicted excess %8.1f us' % (k, t[3], t[0]) +
              ('; measured balance 0 %10.1f us, balance 1 %10.1f us, difference %8.1f us' % (t[1], t[2], t[1] - t[2]) if len(meas) == 2 else ''))


if __name__ == '__main__':
    main()

"""Imputation metrics on the device: per-feature correlation + MSE and per-feature AUROC at the sizes the project imputes.

    python tools/bench_imputation.py [--shapes 8192x128,100000x128,1000000x128,100000x2000] [--host-max 8192] [--check 64]
                                     [--reps 5] [--max-workspace 1073741824] [--peak-tb 8.0]

Per (N, d), on resident inputs, HIP events around the C-ABI calls, one warm-up run, the median of --reps runs:
  stats   jamie_feature_stats: time, the 8 N d bytes it must read over that time, that rate as a share of --peak-tb TB/s, and beside
          it the same share for a device-to-device copy of the same bytes (4 N d read + 4 N d written), measured in the same run;
  auroc   jamie_feature_auroc over all feature groups under --max-workspace, run to the end of stage 1 (key pass), 2 (chunk sort),
          3 (merge passes) and 4 (count): the time of a stage is the difference of two medians, the total is the run to stage 4.
Up to --host-max cells also the wall time of the host `JAMIE(metrics='host').test_imputation` on the same inputs.  On the last
shape --check sampled features are recomputed on the host (np.searchsorted on the sorted negatives) and U2 / n_pos compared.  If
both 100000 x d and 1000000 x d were run, the ratio of their AUROC times is printed against the bound of 20 (N log N predicts
about 12, a quadratic method about 100).  Prints one line per shape and a JSON line at the end."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jamie_amd import _native as nv  # noqa: E402
from jamie_amd import imputation as ji  # noqa: E402

STAGES = ('key pass', 'chunk sort', 'merge passes', 'count')


def timed(fn, reps):
    fn()                                                   # warm-up (code objects, allocator)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
    return statistics.median(ts), min(ts), max(ts)


def host_u2(x, y, thr):
    lab = y > thr
    neg, pos = np.sort(x[~lab]), x[lab]
    return int(np.searchsorted(neg, pos, 'left').sum()) + int(np.searchsorted(neg, pos, 'right').sum()), int(lab.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='8192x128,100000x128,1000000x128,100000x2000')
    ap.add_argument('--host-max', type=int, default=8192)
    ap.add_argument('--check', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--max-workspace', type=int, default=1 << 30)
    ap.add_argument('--peak-tb', type=float, default=8.0, help="the MI355X's HBM bandwidth the shares are taken of, TB/s")
    a = ap.parse_args()
    nv.require_gpu()
    prop = torch.cuda.get_device_properties(0)
    peak = a.peak_tb * 1e12
    print(f'device: {prop.name}, {prop.multi_processor_count} CUs; shares are of {a.peak_tb} TB/s; CHUNK = {ji.CHUNK}, '
          f'workspace cap {a.max_workspace} bytes, median of {a.reps} runs after a warm-up')
    shapes = [tuple(int(v) for v in s.split('x')) for s in a.shapes.split(',')]
    rows = []
    for si, (N, d) in enumerate(shapes):
        p = ji.plan(N, d, a.max_workspace)
        need = 3 * 4 * N * d + max(p['workspace'], nv.imputation_workspace(N, d, 0))
        if need > torch.cuda.mem_get_info()[0]:
            print(f'N={N} d={d}: skipped, inputs and workspace ({need} bytes) do not fit the free device memory')
            continue
        g = torch.Generator(device='cuda').manual_seed(N + d)
        Z = torch.randn(N, d, device='cuda', generator=g)
        X = Z + 1.2 * torch.randn(N, d, device='cuda', generator=g)
        Y = Z + 0.5 * torch.randn(N, d, device='cuda', generator=g)
        Z.copy_(X)                                         # (Z is the copy's destination from here on)
        thr = torch.zeros(d, device='cuda')
        out = torch.empty(2, d, dtype=torch.float64, device='cuda')
        counts = torch.empty(2, d, dtype=torch.int64, device='cuda')
        ws = torch.empty(max(p['workspace'], nv.imputation_workspace(N, d, 0)), dtype=torch.uint8, device='cuda')

        def auroc(last_stage):
            for f0, dg in p['groups']:
                nv.feature_auroc(X, Y, thr, f0, dg, counts[0], counts[1], ws, last_stage)
        t_s = timed(lambda: nv.feature_stats(X, Y, out[0], out[1], ws), a.reps)
        t_c = timed(lambda: Z.copy_(X), a.reps)
        del Z
        prefix = [timed(lambda s=s: auroc(s), a.reps) for s in (1, 2, 3, 4)]
        stage = [prefix[0][0]] + [prefix[i][0] - prefix[i - 1][0] for i in (1, 2, 3)]
        r_dev, mse_dev = out.cpu().numpy()
        n_pos, U2 = counts.cpu().numpy()
        auc = ji.auroc_from_counts(U2, n_pos, N)
        r = {'N': N, 'd': d, 'reps': a.reps, 'groups': len(p['groups']), 'runs': p['runs'], 'merge_passes': p['passes'],
             'workspace_bytes': p['workspace'], 'stats_s': t_s[0], 'stats_s_min_max': t_s[1:], 'stats_bytes_per_s': 8 * N * d / t_s[0],
             'stats_share_of_peak': 8 * N * d / t_s[0] / peak, 'copy_s': t_c[0], 'copy_share_of_peak': 8 * N * d / t_c[0] / peak,
             'auroc_s': prefix[3][0], 'auroc_s_min_max': prefix[3][1:], 'auroc_stage_s': dict(zip(STAGES, stage)),
             'mean_r': float(np.nanmean(r_dev)), 'mean_mse': float(np.nanmean(mse_dev)), 'mean_auroc': float(np.nanmean(auc))}
        line = (f"N={N} d={d}: stats {t_s[0] * 1e3:.3f} ms ({t_s[1] * 1e3:.3f}-{t_s[2] * 1e3:.3f}), {r['stats_bytes_per_s'] / 1e12:.2f} TB/s = "
                f"{r['stats_share_of_peak']:.2f} of peak (a copy of the same bytes: {t_c[0] * 1e3:.3f} ms = {r['copy_share_of_peak']:.2f}); "
                f"auroc {prefix[3][0] * 1e3:.2f} ms ({prefix[3][1] * 1e3:.2f}-{prefix[3][2] * 1e3:.2f}) in {len(p['groups'])} group(s), "
                f"{p['runs']} runs, {p['passes']} merge passes: " + ', '.join(f'{n} {t * 1e3:.2f}' for n, t in zip(STAGES, stage)) +
                f" ms; mean r {r['mean_r']:.4f}, mse {r['mean_mse']:.4f}, auroc {r['mean_auroc']:.4f}")
        if N <= a.host_max:
            from jamie_amd import JAMIE
            hx, hy = X.cpu().numpy(), Y.cpu().numpy()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                host = JAMIE(metrics='host').test_imputation(hx, hy)
            r['host_test_imputation_s'] = time.perf_counter() - t0
            r['host_max_abs_diff'] = {'correlation': float(np.nanmax(np.abs(host['correlation'] - r_dev))),
                                      'mse_relative': float(np.max(np.abs(host['mse'] - mse_dev) / host['mse'])),
                                      'auroc': float(np.nanmax(np.abs(host['auroc'] - auc)))}
            line += (f"; host test_imputation {r['host_test_imputation_s']:.2f} s wall, max difference from the device: r "
                     f"{r['host_max_abs_diff']['correlation']:.1e}, mse (relative) {r['host_max_abs_diff']['mse_relative']:.1e}, auroc "
                     f"{r['host_max_abs_diff']['auroc']:.1e}")
        if si == len(shapes) - 1 and a.check > 0:
            feats = np.sort(np.random.default_rng(0).choice(d, min(a.check, d), replace=False))
            hx, hy = X[:, feats.tolist()].cpu().numpy(), Y[:, feats.tolist()].cpu().numpy()
            same = sum(host_u2(hx[:, k], hy[:, k], np.float32(0)) == (int(U2[f]), int(n_pos[f])) for k, f in enumerate(feats))
            r['cross_check'] = {'features': len(feats), 'equal': int(same)}
            line += f'; cross-check against the host: U2 and n_pos equal on {same} of {len(feats)} sampled features'
        rows.append(r)
        print(line, flush=True)
        del X, Y, ws, out, counts, thr
        torch.cuda.empty_cache()
    verdict = None
    for d in sorted({r['d'] for r in rows}):
        t = {r['N']: r['auroc_s'] for r in rows if r['d'] == d}
        if 100000 in t and 1000000 in t:
            ratio = t[1000000] / t[100000]
            verdict = {'d': d, 'ratio': ratio, 'bound': 20.0, 'met': bool(ratio < 20.0)}
            print(f"auroc time at N = 1000000 over N = 100000, d = {d}: {ratio:.2f}; the bound is 20 (N log N predicts about 12, a "
                  f"quadratic method about 100): {'met' if ratio < 20.0 else 'NOT met'}")
    print(json.dumps({'bench_imputation': rows, 'ratio_condition': verdict, 'peak_bytes_per_s': peak}))


if __name__ == '__main__':
    main()

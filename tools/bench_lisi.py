"""The self neighbour search and LISI on the device: jamie_self_knn on the pooled cells of two modalities at several K, against
jamie_cross_knn(X, X, K + 1) on the same pair space, and jamie_lisi on the lists.

    python tools/bench_lisi.py [--sizes 200000,1000000] [--dims 32,64] [--labels 20] [--host-cells 8192]

Per (pooled N, L): HIP events around the C-ABI calls on resident inputs, median of --reps rounds after one warm-up round.
self_knn at K = 15, 63, 64 and 90; cross_knn(X, X, K + 1) at K = 15 and 63, alternating with self_knn of that K in the same
process: the same pair space and the same list shapes (16 and 64 entries), so the cross search is the yardstick for what the
exclusion by index costs.  K = 64 is the longest single pass, K = 90 the two passes.  jamie_lisi at K = 90, perplexity 30, two
category sets.  Reported: the times, the ratios self / cross and K = 90 / K = 64, and the pair-feature rate N^2 L / t.  Also the
wall time of the host `JAMIE.test_lisi` and of the device one on --host-cells pooled cells.  Prints one line per case and a JSON
line at the end."""
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

SELF_K = (15, 63, 64, 90)
CROSS_K = (15, 63)          # cross_knn runs at K + 1: the cell itself and its K neighbours


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='200000,1000000', help='pooled cells')
    ap.add_argument('--dims', default='32,64')
    ap.add_argument('--labels', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-cells', type=int, default=8192, help='pooled cells of the host test_lisi timing (0: skip)')
    a = ap.parse_args()
    nv.require_gpu()
    prop = torch.cuda.get_device_properties(0)
    print(f'device: {prop.name}, {prop.multi_processor_count} CUs')
    rows = []
    for L in [int(x) for x in a.dims.split(',')]:
        for N in [int(x) for x in a.sizes.split(',')]:
            g = torch.Generator(device='cuda').manual_seed(N + L)
            lab = torch.randint(0, a.labels, (N,), device='cuda', generator=g)
            centres = 2.0 * torch.randn(a.labels, L, device='cuda', generator=g)
            X = centres[lab] + torch.randn(N, L, device='cuda', generator=g)
            X[N // 2:] += 0.3 * torch.randn(N - N // 2, L, device='cuda', generator=g)
            codes = torch.stack([(torch.arange(N, device='cuda') >= N // 2).int(), lab.int()]).contiguous()
            kmax = max(SELF_K)
            idx = torch.empty(N, kmax + 1, dtype=torch.int32, device='cuda')
            dist = torch.empty(N, kmax + 1, dtype=torch.float32, device='cuda')
            need = max([nv.self_knn_workspace(N, k) for k in SELF_K] + [nv.metrics_workspace(N, N, k + 1) for k in CROSS_K])
            ws = torch.empty(need, dtype=torch.uint8, device='cuda')
            out = torch.empty(2, N, dtype=torch.float64, device='cuda')
            tries = torch.empty(N, dtype=torch.int32, device='cuda')
            reps = a.reps if N < 500000 else 3
            work = float(N) * N * L

            def lists(k):
                return idx.view(-1)[:N * k].view(N, k), dist.view(-1)[:N * k].view(N, k)

            def run_self(k):
                i, d = lists(k)
                nv.self_knn(X, k, i, d, ws)

            def run_cross(k):
                i, d = lists(k + 1)
                nv.cross_knn(X, X, k + 1, i, d, ws)

            def run_lisi():
                i, d = lists(90)
                nv.lisi(i, d, codes, 30.0, out, tries)
            r = {'pooled': N, 'L': L, 'reps': reps, 'workspace_bytes': need}
            for k in SELF_K:
                run_self(k)                                # warm-up round (code objects, allocator)
                if k in CROSS_K:
                    run_cross(k)
                torch.cuda.synchronize()
                ts, tc = [], []
                for _ in range(reps):
                    ts.append(event_time(lambda: run_self(k)))
                    if k in CROSS_K:
                        tc.append(event_time(lambda: run_cross(k)))
                r[f'self_knn_k{k}_s'] = statistics.median(ts)
                r[f'self_knn_k{k}_s_min_max'] = (min(ts), max(ts))
                line = (f'N={N}, L={L}: self_knn K={k} {statistics.median(ts) * 1e3:.2f} ms ({min(ts) * 1e3:.2f}-{max(ts) * 1e3:.2f}), '
                        f'{work / statistics.median(ts) / 1e12:.2f} T pair-features/s')
                if k in CROSS_K:
                    r[f'cross_knn_k{k + 1}_s'] = statistics.median(tc)
                    r[f'cross_knn_k{k + 1}_s_min_max'] = (min(tc), max(tc))
                    r[f'self_over_cross_k{k}'] = statistics.median(ts) / statistics.median(tc)
                    line += (f'; cross_knn(X, X, {k + 1}) {statistics.median(tc) * 1e3:.2f} ms ({min(tc) * 1e3:.2f}-'
                             f'{max(tc) * 1e3:.2f}); self / cross {r[f"self_over_cross_k{k}"]:.3f}')
                print(line, flush=True)
            r['k90_over_k64'] = r['self_knn_k90_s'] / r['self_knn_k64_s']
            run_self(90)                                   # (the lists of K = 90 are in place: the last search timed)
            run_lisi()
            torch.cuda.synchronize()
            tl = [event_time(run_lisi) for _ in range(reps)]
            r['lisi_k90_s'] = statistics.median(tl)
            r['lisi_k90_s_min_max'] = (min(tl), max(tl))
            r['mean_tries'] = float(tries.float().mean())
            r['n_failed'] = int(torch.isnan(out[0]).sum())
            print(f"N={N}, L={L}: K=90 / K=64 {r['k90_over_k64']:.3f}; jamie_lisi K=90, 2 sets {r['lisi_k90_s'] * 1e3:.2f} ms "
                  f"({min(tl) * 1e3:.2f}-{max(tl) * 1e3:.2f}), {r['mean_tries']:.1f} tries a cell, {r['n_failed']} failed; iLISI median "
                  f"{float(out[0].nanmedian()):.4f}, cLISI median {float(out[1].nanmedian()):.4f}; workspace {need / 2 ** 20:.0f} MiB",
                  flush=True)
            rows.append(r)
            del X, idx, dist, ws, out, tries, codes, lab, centres
            torch.cuda.empty_cache()
    host = None
    if a.host_cells > 0:
        from jamie_amd import JAMIE
        n, L = a.host_cells // 2, 32
        rng = np.random.default_rng(0)
        labs = [rng.integers(0, a.labels, n) for _ in range(2)]
        centres = 2.0 * rng.standard_normal((a.labels, L))
        emb = [(centres[lab] + rng.standard_normal((n, L)) + 0.2 * m).astype(np.float32).astype(np.float64)
               for m, lab in enumerate(labs)]
        res = {}
        for mode in ('device', 'device', 'host'):          # (the first device call also loads the code objects)
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                res[mode] = JAMIE(metrics=mode).test_lisi(emb, labs)
            torch.cuda.synchronize()
            res[mode + '_s'] = time.perf_counter() - t0
        rel = np.abs(res['host']['ilisi'] - res['device']['ilisi']) / res['host']['ilisi']
        host = {'pooled': 2 * n, 'L': L, 'host_test_lisi_s': res['host_s'], 'device_test_lisi_s': res['device_s'],
                'ilisi_median': (res['host']['ilisi_median'], res['device']['ilisi_median']),
                'clisi_median': (res['host']['clisi_median'], res['device']['clisi_median']),
                'median_relative_ilisi_difference': float(np.median(rel))}
        print(f"test_lisi on {2 * n} pooled cells, L={L}: host {res['host_s']:.2f} s wall, device {res['device_s']:.3f} s wall; iLISI "
              f"median {host['ilisi_median'][0]:.6f} / {host['ilisi_median'][1]:.6f}, cLISI median {host['clisi_median'][0]:.6f} / "
              f"{host['clisi_median'][1]:.6f}")
    print(json.dumps({'bench_lisi': rows, 'test_lisi': host}))


if __name__ == '__main__':
    main()

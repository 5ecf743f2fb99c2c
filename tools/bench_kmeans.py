"""k-means on the device: the fused Lloyd step (jamie_kmeans_step: assignment, fp64 cluster sums, new centres and the stop rules
in one pass over X) against the assignment alone by the cross search, and against a copy of X.

    python tools/bench_kmeans.py [--sizes 200000,1000000] [--dims 32,64] [--clusters 40,256] [--host-cells 8192] [--log PATH]

Per (pooled N, L, k): HIP events around the C-ABI calls on resident inputs, median of --reps rounds (3 at 10^6 cells) after one
warm-up round.  jamie_cross_knn(X, C, K = 1) alternates with the step in the same process on the same X and C: it is the
assignment alone.  The copy is a device copy of X's bytes.  Reported: the step's time, its ratio to the cross search, the
fraction of 8 TB/s the step reaches on the 4 N L bytes it must read beside the copy's (which reads and writes them), the wall time
and the iterations of a whole `clustering.kmeans` call (n_init = 1), and the wall time of sklearn's KMeans from the same centres on
--host-cells cells.  Prints one line per case, a JSON line at the end, and writes both to --log."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jamie_amd import _native as nv  # noqa: E402
from jamie_amd import clustering as jc  # noqa: E402

HBM = 8e12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    ap.add_argument('--clusters', default='40,256')
    ap.add_argument('--blobs', type=int, default=40)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-cells', type=int, default=8192, help='cells of the sklearn KMeans timing (0: skip)')
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'bench_kmeans.log'))
    a = ap.parse_args()
    nv.require_gpu()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    say(f'device: {prop.name}, {prop.multi_processor_count} CUs')
    rows = []
    for L in [int(x) for x in a.dims.split(',')]:
        for N in [int(x) for x in a.sizes.split(',')]:
            g = torch.Generator(device='cuda').manual_seed(N + L)
            lab = torch.randint(0, a.blobs, (N,), device='cuda', generator=g)
            X = 2.0 * torch.randn(a.blobs, L, device='cuda', generator=g)[lab] + torch.randn(N, L, device='cuda', generator=g)
            del lab
            copy = torch.empty_like(X)
            reps = a.reps if N < 500000 else 3
            event_time(lambda: copy.copy_(X))
            tcopy = statistics.median([event_time(lambda: copy.copy_(X)) for _ in range(reps)])
            del copy
            for k in [int(x) for x in a.clusters.split(',')]:
                C = X[torch.randperm(N, device='cuda', generator=g)[:k]].clone()
                labels = torch.full((N,), -1, dtype=torch.int32, device='cuda')
                counts = torch.empty(k, dtype=torch.int64, device='cuda')
                stats = torch.zeros(4, dtype=torch.float64, device='cuda')
                state = torch.zeros(4, dtype=torch.int32, device='cuda')
                ws = torch.empty(nv.kmeans_workspace(N, L, k), dtype=torch.uint8, device='cuda')
                idx = torch.empty(N, 1, dtype=torch.int32, device='cuda')
                dist = torch.empty(N, 1, dtype=torch.float32, device='cuda')
                cws = torch.empty(nv.metrics_workspace(N, k, 1), dtype=torch.uint8, device='cuda')

                def run_step():
                    nv.kmeans_step(X, C, labels, counts, stats, state, ws, 0.0, 1 << 30, False)

                def run_cross():
                    nv.cross_knn(X, C, 1, idx, dist, cws)
                run_step()
                run_cross()
                torch.cuda.synchronize()
                ts, tc = [], []
                for _ in range(reps):
                    state.zero_()                          # (the centres stay: the labels repeat, which would raise `done`)
                    ts.append(event_time(run_step))
                    tc.append(event_time(run_cross))
                same = bool((labels == idx[:, 0]).all())
                del idx, dist, cws, ws, labels
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                km = jc.kmeans(X, k, n_init=1, seed=0)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                t_step, t_cross = statistics.median(ts), statistics.median(tc)
                r = {'pooled': N, 'L': L, 'k': k, 'reps': reps, 'step_s': t_step, 'step_s_min_max': (min(ts), max(ts)),
                     'cross_knn_k1_s': t_cross, 'cross_knn_k1_s_min_max': (min(tc), max(tc)), 'step_over_cross': t_step / t_cross,
                     'copy_s': tcopy, 'step_fraction_of_hbm': 4.0 * N * L / t_step / HBM, 'copy_fraction_of_hbm': 4.0 * N * L / tcopy / HBM,
                     'pair_features_per_s': float(N) * k * L / t_step, 'labels_equal_cross_knn': same,
                     'workspace_bytes': nv.kmeans_workspace(N, L, k), 'kmeans_wall_s': wall, 'kmeans_n_iter': km['n_iter'],
                     'kmeans_converged': km['converged']}
                say(f"N={N}, L={L}, k={k}: step {t_step * 1e3:.3f} ms ({min(ts) * 1e3:.3f}-{max(ts) * 1e3:.3f}); cross_knn(X, C, 1) "
                    f"{t_cross * 1e3:.3f} ms ({min(tc) * 1e3:.3f}-{max(tc) * 1e3:.3f}); step / cross {r['step_over_cross']:.3f}; "
                    f"{r['pair_features_per_s'] / 1e12:.2f} T pair-features/s; {r['step_fraction_of_hbm']:.4f} of 8 TB/s on 4NL bytes "
                    f"(copy {tcopy * 1e3:.3f} ms, {r['copy_fraction_of_hbm']:.4f}); labels equal the search's: {same}; kmeans "
                    f"(n_init 1) {wall:.3f} s wall, {km['n_iter']} iterations, converged {km['converged']}; workspace "
                    f"{r['workspace_bytes'] / 2 ** 20:.1f} MiB")
                rows.append(r)
            del X
            torch.cuda.empty_cache()
    host = None
    if a.host_cells > 0:
        from sklearn.cluster import KMeans
        n, L, k = a.host_cells, 32, 40
        rng = np.random.default_rng(0)
        X = (2.0 * rng.standard_normal((a.blobs, L))[rng.integers(0, a.blobs, n)] + rng.standard_normal((n, L))).astype(np.float32)
        init = X[rng.permutation(n)[:k]]
        t0 = time.perf_counter()
        sk = KMeans(n_clusters=k, init=init.astype(np.float64), n_init=1, algorithm='lloyd').fit(X.astype(np.float64))
        t_sk = time.perf_counter() - t0
        res = {}
        for mode in ('first', 'second'):                   # (the first device call also loads the code objects)
            t0 = time.perf_counter()
            res[mode] = jc.kmeans(X, k, init=init)
            torch.cuda.synchronize()
            res[mode + '_s'] = time.perf_counter() - t0
        host = {'cells': n, 'L': L, 'k': k, 'sklearn_s': t_sk, 'sklearn_n_iter': int(sk.n_iter_), 'sklearn_inertia': float(sk.inertia_),
                'device_s': res['second_s'], 'device_n_iter': res['second']['n_iter'], 'device_inertia': res['second']['inertia']}
        say(f"{n} cells, L={L}, k={k}, the same initial centres: sklearn KMeans (lloyd) {t_sk:.3f} s wall, {host['sklearn_n_iter']} "
            f"iterations, inertia {host['sklearn_inertia']:.6g}; clustering.kmeans {host['device_s']:.3f} s wall, "
            f"{host['device_n_iter']} iterations, inertia {host['device_inertia']:.6g}")
    say(json.dumps({'bench_kmeans': rows, 'sklearn': host}))
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

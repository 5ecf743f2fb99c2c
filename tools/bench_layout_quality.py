"""Layout quality on the device: jamie_list_ranks on resident inputs, against jamie_foscttm_counts and jamie_self_knn on the same
pair space.

    python tools/bench_layout_quality.py [--sizes 200000,1000000] [--dims 32,2] [--ks 15,64] [--reps 5]

Per (pooled N, L, K): HIP events around the C-ABI calls, median of --reps rounds (3 from 500 000 cells) after one warm-up round,
the calls alternating in the same process.  X is a gaussian mixture [N, L]; the lists ranked in it are the self_knn lists of a second space,
once a FAITHFUL one (a linear projection of X to max(L / 2, min(L, 2)) dimensions plus small noise: most ranks stay near K) and
once a RANDOM one (ranks up to N: the slow path sees a large share of the pairs); and X's OWN lists (ranks 0 .. K - 1: the slow
path sees K of N pairs, so this is the cost of the tile loop with its one test per row of 8 pairs).  The yardstick is
jamie_foscttm_counts(X, X): the same tile over the same pair space with one compare per pair.  Reported: the times, the ratios
list_ranks / foscttm for the regimes and list_ranks / self_knn(K), the largest and the mean rank of each regime, and the device
time of the whole `neighborhood_preservation`.  Prints one line per case and a JSON line at the end; the log kept with the repository is
profiles/bench_layout_quality.log."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jamie_amd import _native as nv  # noqa: E402


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
    ap.add_argument('--dims', default='32,2')
    ap.add_argument('--ks', default='15,64')
    ap.add_argument('--labels', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    nv.require_gpu()
    from jamie_amd import coranking
    prop = torch.cuda.get_device_properties(0)
    print(f'device: {prop.name}, {prop.multi_processor_count} CUs')
    rows = []
    for L in [int(x) for x in a.dims.split(',')]:
        for N in [int(x) for x in a.sizes.split(',')]:
            g = torch.Generator(device='cuda').manual_seed(N + L)
            lab = torch.randint(0, a.labels, (N,), device='cuda', generator=g)
            X = (2.0 * torch.randn(a.labels, L, device='cuda', generator=g))[lab] + torch.randn(N, L, device='cuda', generator=g)
            Lf = max(L // 2, min(L, 2))
            faithful = X @ torch.randn(L, Lf, device='cuda', generator=g) / L ** 0.5
            faithful += 0.01 * faithful.std() * torch.randn(N, Lf, device='cuda', generator=g)
            random = torch.randn(N, 2, device='cuda', generator=g)
            reps = a.reps if N < 500000 else 3
            for K in [int(x) for x in a.ks.split(',')]:
                idx = {name: torch.empty(N, K, dtype=torch.int32, device='cuda') for name in ('faithful', 'random')}
                dist = torch.empty(N, K, dtype=torch.float32, device='cuda')
                own = torch.empty(N, K, dtype=torch.int32, device='cuda')
                rank = torch.empty(N, K, dtype=torch.int32, device='cuda')
                counts = torch.empty(2, N, dtype=torch.int32, device='cuda')
                need = max(nv.self_knn_workspace(N, K), nv.list_ranks_workspace(N, K), nv.metrics_workspace(N, N, 0))
                ws = torch.empty(need, dtype=torch.uint8, device='cuda')
                nv.self_knn(faithful, K, idx['faithful'], dist, ws)
                nv.self_knn(random, K, idx['random'], dist, ws)
                calls = {'foscttm': lambda: nv.foscttm_counts(X, X, counts[0], counts[1], ws),
                         'self_knn': lambda: nv.self_knn(X, K, own, dist, ws),
                         'ranks_own': lambda: nv.list_ranks(X, own, rank, ws),
                         'ranks_faithful': lambda: nv.list_ranks(X, idx['faithful'], rank, ws),
                         'ranks_random': lambda: nv.list_ranks(X, idx['random'], rank, ws)}
                for fn in calls.values():                  # warm-up round (code objects, allocator)
                    fn()
                torch.cuda.synchronize()
                times = {name: [] for name in calls}
                top = {}
                for _ in range(reps):
                    for name, fn in calls.items():
                        times[name].append(event_time(fn))
                        if name.startswith('ranks_'):
                            top[name] = (int(rank.max()), float(rank.float().mean()))
                med = {name: statistics.median(t) for name, t in times.items()}
                r = {'pooled': N, 'L': L, 'K': K, 'reps': reps, 'faithful_dims': Lf,
                     **{name + '_s': med[name] for name in calls},
                     **{name + '_s_min_max': (min(times[name]), max(times[name])) for name in calls},
                     'faithful_over_foscttm': med['ranks_faithful'] / med['foscttm'],
                     'random_over_foscttm': med['ranks_random'] / med['foscttm'],
                     'faithful_over_self_knn': med['ranks_faithful'] / med['self_knn'],
                     'own_over_foscttm': med['ranks_own'] / med['foscttm'],
                     'largest_and_mean_rank_faithful': top['ranks_faithful'], 'largest_and_mean_rank_random': top['ranks_random']}
                print(f"N={N}, L={L}, K={K}: foscttm {med['foscttm'] * 1e3:.2f} ms, self_knn {med['self_knn'] * 1e3:.2f} ms, list_ranks own "
                      f"{med['ranks_own'] * 1e3:.2f} ms, "
                      f"faithful {med['ranks_faithful'] * 1e3:.2f} ms ({min(times['ranks_faithful']) * 1e3:.2f}-"
                      f"{max(times['ranks_faithful']) * 1e3:.2f}; largest, mean rank {top['ranks_faithful'][0]}, {top['ranks_faithful'][1]:.1f}), random "
                      f"{med['ranks_random'] * 1e3:.2f} ms ({min(times['ranks_random']) * 1e3:.2f}-{max(times['ranks_random']) * 1e3:.2f}; "
                      f"mean rank {top['ranks_random'][1]:.0f}); ranks / foscttm {r['own_over_foscttm']:.3f} own, {r['faithful_over_foscttm']:.3f} faithful, "
                      f"{r['random_over_foscttm']:.3f} random; ranks / self_knn {r['faithful_over_self_knn']:.3f}", flush=True)
                rows.append(r)
                del idx, dist, own, rank, counts, ws
            # the whole metric on the faithful pair of spaces, resident inputs
            coranking.neighborhood_preservation([X], [faithful], n_neighbors=15)
            t = [event_time(lambda: coranking.neighborhood_preservation([X], [faithful], n_neighbors=15)) for _ in range(2)]
            out = coranking.neighborhood_preservation([X], [faithful], n_neighbors=15)
            print(f"N={N}, L={L}: neighborhood_preservation K=15 {min(t):.3f} s; trustworthiness {out['trustworthiness']:.4f}, "
                  f"continuity {out['continuity']:.4f}, k_best {out['k_best']}", flush=True)
            rows.append({'pooled': N, 'L': L, 'neighborhood_preservation_k15_s': min(t), 'trustworthiness': out['trustworthiness'],
                         'continuity': out['continuity']})
            del X, faithful, random, lab
            torch.cuda.empty_cache()
    print(json.dumps({'bench_layout_quality': rows}))


if __name__ == '__main__':
    main()

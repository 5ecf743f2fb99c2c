"""Stage A (geodesic distances of one modality) on the host and on the device.

    python tools/bench_geodesic.py [--sizes 2048,4096,8192,16384] [--dims 64,2000] [--host-max 8192] [--kmax 40]

Per (N, d): end-to-end seconds from a host float64 array to the device result (device path: jamie_amd.distances.geodesic,
after one warm-up call; host path: utilities.geodesic_distances, up to --host-max cells), the device time of every stage (HIP
events around each C-ABI call, the growth loop's host connectivity test included in 'growth loop') and the Floyd-Warshall rate
in (i, j, k) triples per second over the whole jamie_apsp_fw call (phases 1-3; rocprofv3 --kernel-trace --stats gives phase 3
alone).  Prints one line per size and a JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jamie_amd import _native as nv  # noqa: E402
from jamie_amd import distances as jd  # noqa: E402


def staged(X, kmax):
    """jd.geodesic step by step, each stage timed on the device."""
    ev = []

    def mark():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        ev.append(e)
    mark()
    Xc = jd.centred(X)
    mark()
    N = Xc.shape[0]
    K = jd.k_max(N, kmax)
    D = jd._euclidean_centred(Xc)
    mark()
    idx = torch.empty(N, K, dtype=torch.int32, device='cuda')
    w = torch.empty(N, K, dtype=torch.float32, device='cuda')
    nv.knn_topk(D, K, idx)
    mark()
    nv.knn_weights(Xc, idx, w)
    mark()
    ih = idx.cpu().numpy()
    k = jd.K_MIN
    while not jd._connected(ih, min(k, N)):
        if k > np.max((kmax, 0.01 * N)):
            break
        k += 2
    k = min(k, N)
    mark()
    nv.knn_graph_init(D, idx, w, k)
    mark()
    nv.apsp_fw(D)
    mark()
    partials = torch.empty(nv.dist_workspace(N), dtype=torch.float32, device='cuda')
    maxv = torch.empty(1, dtype=torch.float32, device='cuda')
    nv.apsp_finalise(D, partials, maxv)
    mark()
    torch.cuda.synchronize()
    names = ['upload + centre', 'gram + distances', 'top-K', 'edge weights', 'growth loop', 'graph init', 'floyd-warshall',
             'finalise']
    return {n: ev[i].elapsed_time(ev[i + 1]) / 1e3 for i, n in enumerate(names)}, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='2048,4096,8192,16384')
    ap.add_argument('--dims', default='64,2000')
    ap.add_argument('--host-max', type=int, default=8192)
    ap.add_argument('--kmax', type=int, default=40)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    nv.require_gpu()
    print('device:', torch.cuda.get_device_name(0))
    rows = []
    for d in [int(x) for x in a.dims.split(',')]:
        for N in [int(x) for x in a.sizes.split(',')]:
            rng = np.random.default_rng(N + d)
            X = rng.standard_normal((N, d))
            jd.geodesic(X, a.kmax)                        # warm-up (code objects, allocator)
            torch.cuda.synchronize()
            e2e = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                D = jd.geodesic(X, a.kmax)
                torch.cuda.synchronize()
                e2e.append(time.perf_counter() - t0)
                del D
            stages, k = staged(X, a.kmax)
            fw = stages['floyd-warshall']
            r = {'N': N, 'd': d, 'k': k, 'device_s': min(e2e), 'stages_s': stages, 'fw_triples_per_s': N ** 3 / fw}
            if N <= a.host_max:
                from jamie_amd.utilities import geodesic_distances
                t0 = time.perf_counter()
                H = geodesic_distances(X, a.kmax)
                t1 = time.perf_counter()
                Dd = jd.geodesic(X, a.kmax).cpu().numpy()
                r['host_s'] = t1 - t0
                r['max_rel_err_vs_host'] = float(np.abs(Dd - H).max() / H.max())
            rows.append(r)
            st = ' '.join(f'{n}={v * 1e3:.2f}ms' for n, v in stages.items())
            print(f"N={N} d={d} k={k}: device {r['device_s']:.3f} s"
                  + (f", host {r['host_s']:.2f} s, max |dD|/max D {r['max_rel_err_vs_host']:.1e}" if 'host_s' in r else '')
                  + f"; FW {r['fw_triples_per_s'] / 1e12:.2f} Ttriples/s; {st}", flush=True)
    print(json.dumps({'bench_geodesic': rows}))


if __name__ == '__main__':
    main()

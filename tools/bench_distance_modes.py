"""Stage A on the device for the correlation family and the L1 family: time per mode next to `euclidean` and to the host path.

    python tools/bench_distance_modes.py [--n 8192] [--dims 64,2000] [--reps 5] [--host-n 8192] [--clock-ghz 2.4]

Per d, on one resident fp32 [N, d] device tensor of N(0, 1) + 1: the device time of every public function of
jamie_amd/distances.py for the new modes and of `euclidean` (HIP events around the call: input check, unit rows or centring, Gram
product, distance pass; median of --reps runs after one warm-up run), and for the L1 family also of jamie_pairwise_absdiff alone with
its pair-feature rate N^2 d / 2 / t (the kernel walks the tiles I <= J only) as a share of the fp32 VALU issue ceiling: one v_sub_f32
+ one v_add_f32 (v_max_f32) per pair and feature, a wave64 instruction every 2 cycles per SIMD, so CUs x 4 SIMDs x 32 lanes x
clock / 2 pair-features per second.  Then the wall time of the host `utilities.distance_matrix` for the same mode on the first
--host-n cells of the same data (float64, one run).  Prints one line per mode and a JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jamie_amd import _native as nv  # noqa: E402
from jamie_amd import distances as jd  # noqa: E402

MODES = ('euclidean', 'cosine', 'correlation', 'pearson', 'manhattan', 'chebyshev')


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--dims', default='64,2000')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-n', type=int, default=8192, help='cells of the host timing (0: no host timing)')
    ap.add_argument('--clock-ghz', type=float, default=2.4, help="the ceiling's clock: the MI355X's peak engine clock")
    a = ap.parse_args()
    nv.require_gpu()
    from jamie_amd.utilities import distance_matrix
    prop = torch.cuda.get_device_properties(0)
    ceiling = prop.multi_processor_count * 4 * 32 * a.clock_ghz * 1e9 / 2
    print(f'device: {prop.name}, {prop.multi_processor_count} CUs at {a.clock_ghz:.2f} GHz: fp32 VALU issue ceiling '
          f'{ceiling / 1e12:.1f} T pair-features/s (sub + add per pair and feature)')
    N, rows = a.n, []
    for d in [int(x) for x in a.dims.split(',')]:
        g = torch.Generator(device='cuda').manual_seed(N + d)
        X = torch.randn(N, d, device='cuda', generator=g) + 1.0
        D = torch.empty(N, N, dtype=torch.float32, device='cuda')
        host = X[:min(a.host_n, N)].cpu().numpy().astype('float64')
        for mode in MODES:
            t = timed(lambda: getattr(jd, mode)(X), a.reps)
            r = {'mode': mode, 'N': N, 'd': d, 'reps': a.reps, 'device_s': t[0], 'device_s_min_max': t[1:]}
            line = f'N={N} d={d} {mode}: device {t[0] * 1e3:.2f} ms ({t[1] * 1e3:.2f}-{t[2] * 1e3:.2f})'
            if mode in ('manhattan', 'chebyshev'):
                tk = timed(lambda: nv.pairwise_absdiff(X, int(mode == 'chebyshev'), D), a.reps)
                r.update(kernel_s=tk[0], kernel_s_min_max=tk[1:], pair_features_per_s=N * N * d / 2 / tk[0],
                         share_of_ceiling=N * N * d / 2 / tk[0] / ceiling)
                line += (f', jamie_pairwise_absdiff alone {tk[0] * 1e3:.2f} ms ({tk[1] * 1e3:.2f}-{tk[2] * 1e3:.2f}): '
                         f"{r['pair_features_per_s'] / 1e12:.2f} T pair-features/s = {r['share_of_ceiling']:.0%} of the ceiling")
            if len(host):
                t0 = time.perf_counter()
                distance_matrix(host, mode)
                r.update(host_s=time.perf_counter() - t0, host_N=len(host))
                line += f"; host distance_matrix on {len(host)} cells {r['host_s']:.2f} s wall"
            rows.append(r)
            print(line, flush=True)
        del X, D
        torch.cuda.empty_cache()
    print(json.dumps({'bench_distance_modes': rows, 'ceiling_pair_features_per_s': ceiling}))


if __name__ == '__main__':
    main()

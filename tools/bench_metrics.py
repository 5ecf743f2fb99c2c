"""Alignment metrics on the device: FOSCTTM and k = 5 label transfer at the sizes the project trains.

    python tools/bench_metrics.py [--sizes 8192,100000,1000000] [--dims 32,64] [--host-max 8192] [--k 5] [--classes 12] [--clock-ghz 2.4]

Per (N, L): the device time of jamie_foscttm_counts and of jamie_cross_knn + jamie_knn_vote from HIP events around the C-ABI
calls on resident inputs (median of --reps runs after one warm-up run), the pair-feature rate N^2 L / t, and that rate as a
share of the fp32 VALU issue ceiling the kernels are bound by: one v_sub_f32 + one v_fma_f32 per pair and feature, a wave64
instruction every 2 cycles per SIMD, so CUs x 4 SIMDs x 32 lanes x clock / 2 pair-features per second.  Up to --host-max cells
also the wall time of the host `JAMIE.test_closer` on the same inputs.  Prints one line per size and a JSON line at the end."""
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
from jamie_amd import metrics as jm  # noqa: E402


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
    ap.add_argument('--sizes', default='8192,100000,1000000')
    ap.add_argument('--dims', default='32,64')
    ap.add_argument('--host-max', type=int, default=8192)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--classes', type=int, default=12)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--clock-ghz', type=float, default=2.4, help="the ceiling's clock: the MI355X's peak engine clock")
    a = ap.parse_args()
    nv.require_gpu()
    prop = torch.cuda.get_device_properties(0)
    clock = a.clock_ghz * 1e9
    ceiling = prop.multi_processor_count * 4 * 32 * clock / 2
    print(f'device: {prop.name}, {prop.multi_processor_count} CUs at {clock / 1e9:.2f} GHz: fp32 VALU issue ceiling '
          f'{ceiling / 1e12:.1f} T pair-features/s (sub + fma per pair and feature)')
    free = torch.cuda.mem_get_info()[0]
    rows = []
    for L in [int(x) for x in a.dims.split(',')]:
        for N in [int(x) for x in a.sizes.split(',')]:
            if 4 * N * L * 4 > free:
                print(f'N={N} L={L}: skipped, the inputs do not fit the free device memory')
                continue
            g = torch.Generator(device='cuda').manual_seed(N + L)
            Z = torch.randn(N, L, device='cuda', generator=g)
            A = Z + 1.5 * torch.randn(N, L, device='cuda', generator=g)
            B = Z + 1.5 * torch.randn(N, L, device='cuda', generator=g)
            del Z
            codes = torch.randint(0, a.classes, (N,), device='cuda', generator=g).to(torch.int32)
            reps = a.reps if N < 500000 else 3
            counts = torch.empty(2, N, dtype=torch.int32, device='cuda')
            ws = torch.empty(max(nv.metrics_workspace(N, N, 0), nv.metrics_workspace(N, N, a.k)), dtype=torch.uint8, device='cuda')
            idx = torch.empty(N, a.k, dtype=torch.int32, device='cuda')
            dist = torch.empty(N, a.k, dtype=torch.float32, device='cuda')
            pred = torch.empty(N, dtype=torch.int32, device='cuda')

            def run_lta():
                nv.cross_knn(A, B, a.k, idx, dist, ws)
                nv.knn_vote(idx, codes, a.classes, pred)
            t_f = timed(lambda: nv.foscttm_counts(A, B, counts[0], counts[1], ws), reps)
            value = int(counts.sum(dtype=torch.int64)) / (2 * N ** 2)
            t_k = timed(run_lta, reps)
            r = {'N': N, 'L': L, 'k': a.k, 'reps': reps, 'foscttm': value,
                 'foscttm_s': t_f[0], 'foscttm_s_min_max': t_f[1:], 'foscttm_pair_features_per_s': N * N * L / t_f[0],
                 'foscttm_share_of_ceiling': N * N * L / t_f[0] / ceiling,
                 'label_transfer_s': t_k[0], 'label_transfer_s_min_max': t_k[1:],
                 'label_transfer_pair_features_per_s': N * N * L / t_k[0],
                 'label_transfer_share_of_ceiling': N * N * L / t_k[0] / ceiling}
            line = (f"N={N} L={L}: foscttm {value:.6f} in {t_f[0] * 1e3:.2f} ms ({t_f[1] * 1e3:.2f}-{t_f[2] * 1e3:.2f}), "
                    f"{r['foscttm_pair_features_per_s'] / 1e12:.2f} T pair-features/s = {r['foscttm_share_of_ceiling']:.0%} of the "
                    f"ceiling; label transfer k={a.k} in {t_k[0] * 1e3:.2f} ms ({t_k[1] * 1e3:.2f}-{t_k[2] * 1e3:.2f}), "
                    f"{r['label_transfer_pair_features_per_s'] / 1e12:.2f} T pair-features/s = "
                    f"{r['label_transfer_share_of_ceiling']:.0%}")
            if N <= a.host_max:
                from jamie_amd import JAMIE
                e0, e1 = A.cpu().numpy().astype(np.float64), B.cpu().numpy().astype(np.float64)
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    host = JAMIE().test_closer([e0, e1])
                r['host_test_closer_s'] = time.perf_counter() - t0
                r['host_foscttm'] = float(host)
                line += f"; host test_closer {r['host_test_closer_s']:.2f} s wall, foscttm {host:.6f}"
            rows.append(r)
            print(line, flush=True)
            del A, B, counts, ws, idx, dist, pred, codes
            torch.cuda.empty_cache()
    print(json.dumps({'bench_metrics': rows, 'ceiling_pair_features_per_s': ceiling}))


if __name__ == '__main__':
    main()

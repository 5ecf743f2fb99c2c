"""Silhouette widths on the device: jamie_label_distance_sums on the pooled cells of two modalities, against FOSCTTM on the same
pair space.

    python tools/bench_silhouette.py [--sizes 100000,500000] [--dims 32,64] [--labels 20] [--host-cells 8192] [--clock-ghz 2.4]

Per (N cells a modality, L): the 2 N pooled cells are queries and (sorted by class code label * 2 + modality) reference rows of
one jamie_label_distance_sums call, S [2 N, 2 labels] fp64.  jamie_foscttm_counts on two embeddings of 2 N cells walks a pair
space of the same size; the two are timed alternating in one process, HIP events around the C-ABI calls on resident inputs,
median of --reps rounds after one warm-up round.  Reported: both times, the pair-feature rates (2 N)^2 L / t, their ratio, and
the rate as a share of the fp32 VALU issue ceiling of the sub + fma per pair and feature (tools/bench_metrics.py).  Also the
wall time of the host `JAMIE.test_silhouette` and of the device one on --host-cells pooled cells.  Prints one line per case and
a JSON line at the end."""
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


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='100000,500000', help='cells per modality')
    ap.add_argument('--dims', default='32,64')
    ap.add_argument('--labels', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-cells', type=int, default=8192, help='pooled cells of the host test_silhouette timing (0: skip)')
    ap.add_argument('--clock-ghz', type=float, default=2.4, help="the ceiling's clock: the MI355X's peak engine clock")
    a = ap.parse_args()
    nv.require_gpu()
    prop = torch.cuda.get_device_properties(0)
    ceiling = prop.multi_processor_count * 4 * 32 * a.clock_ghz * 1e9 / 2
    print(f'device: {prop.name}, {prop.multi_processor_count} CUs at {a.clock_ghz:.2f} GHz: fp32 VALU issue ceiling '
          f'{ceiling / 1e12:.1f} T pair-features/s (sub + fma per pair and feature)')
    rows = []
    M = 2
    for L in [int(x) for x in a.dims.split(',')]:
        for N in [int(x) for x in a.sizes.split(',')]:
            P, C = M * N, M * a.labels
            g = torch.Generator(device='cuda').manual_seed(N + L)
            lab = torch.randint(0, a.labels, (P,), device='cuda', generator=g)
            centres = 2.0 * torch.randn(a.labels, L, device='cuda', generator=g)
            X = centres[lab] + torch.randn(P, L, device='cuda', generator=g)
            X[N:] += 0.3 * torch.randn(P - N, L, device='cuda', generator=g)
            Y = X + 1.5 * torch.randn(P, L, device='cuda', generator=g)          # FOSCTTM's second embedding of the P cells
            code = (lab * M + (torch.arange(P, device='cuda') >= N).long()).cpu().numpy()
            Xs, off, counts = jm._sorted_by_class(X, code, C)
            S = torch.empty(P, C, dtype=torch.float64, device='cuda')
            ws = torch.empty(nv.label_sums_workspace(P, P, C, 0), dtype=torch.uint8, device='cuda')
            fc = torch.empty(2, P, dtype=torch.int32, device='cuda')
            fws = torch.empty(nv.metrics_workspace(P, P, 0), dtype=torch.uint8, device='cuda')
            reps = a.reps if P < 500000 else 3

            def sil():
                nv.label_distance_sums(X, Xs, off, S, ws)

            def fos():
                nv.foscttm_counts(X, Y, fc[0], fc[1], fws)
            sil(), fos()                                   # warm-up round (code objects, allocator)
            torch.cuda.synchronize()
            ts, tf = [], []
            for _ in range(reps):
                ts.append(event_time(sil))
                tf.append(event_time(fos))
            t_s, t_f = statistics.median(ts), statistics.median(tf)
            work = float(P) * P * L
            r = {'cells_per_modality': N, 'pooled': P, 'L': L, 'classes': C, 'reps': reps,
                 'workspace_bytes': ws.numel(), 'S_bytes': S.numel() * 8,
                 'label_sums_s': t_s, 'label_sums_s_min_max': (min(ts), max(ts)), 'label_sums_pair_features_per_s': work / t_s,
                 'label_sums_share_of_ceiling': work / t_s / ceiling,
                 'foscttm_s': t_f, 'foscttm_s_min_max': (min(tf), max(tf)), 'foscttm_pair_features_per_s': work / t_f,
                 'foscttm_share_of_ceiling': work / t_f / ceiling, 'rate_ratio_to_foscttm': t_f / t_s}
            rows.append(r)
            print(f"N={N} x 2 modalities (pooled {P}), L={L}, {C} classes: label distance sums {t_s * 1e3:.2f} ms "
                  f"({min(ts) * 1e3:.2f}-{max(ts) * 1e3:.2f}), {work / t_s / 1e12:.2f} T pair-features/s = "
                  f"{r['label_sums_share_of_ceiling']:.0%} of the ceiling; foscttm on {P} cells {t_f * 1e3:.2f} ms "
                  f"({min(tf) * 1e3:.2f}-{max(tf) * 1e3:.2f}), {work / t_f / 1e12:.2f} T pair-features/s = "
                  f"{r['foscttm_share_of_ceiling']:.0%}; rate ratio to foscttm {t_f / t_s:.3f}; workspace "
                  f"{ws.numel() / 2 ** 20:.0f} MiB + S {S.numel() * 8 / 2 ** 20:.0f} MiB", flush=True)
            del X, Y, Xs, S, ws, fc, fws, lab, centres
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
        out = {}
        for mode in ('device', 'device', 'host'):          # (the first device call also loads the code objects)
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                out[mode] = JAMIE(metrics=mode).test_silhouette(emb, labs)
            torch.cuda.synchronize()
            out[mode + '_s'] = time.perf_counter() - t0
        host = {'pooled': 2 * n, 'L': L, 'host_test_silhouette_s': out['host_s'], 'device_test_silhouette_s': out['device_s'],
                'label_asw': (out['host']['label_asw'], out['device']['label_asw']),
                'modality_asw': (out['host']['modality_asw'], out['device']['modality_asw']),
                'max_width_difference': float(np.abs(out['host']['label_widths'] - out['device']['label_widths']).max())}
        print(f"test_silhouette on {2 * n} pooled cells, L={L}: host {out['host_s']:.2f} s wall, device {out['device_s']:.3f} s wall; "
              f"label ASW {host['label_asw'][0]:.6f} / {host['label_asw'][1]:.6f}, modality ASW {host['modality_asw'][0]:.6f} / "
              f"{host['modality_asw'][1]:.6f}, widths differ by at most {host['max_width_difference']:.2e}")
    print(json.dumps({'bench_silhouette': rows, 'test_silhouette': host, 'ceiling_pair_features_per_s': ceiling}))


if __name__ == '__main__':
    main()

"""Marker features on the device: the moments pass and the rank-sum pass of `rank_features` at the sizes the project imputes.

    python tools/bench_markers.py [--shapes 100000x2000x40,1000000x128x40] [--host-shape 8192x128x40] [--check 16] [--reps 5]
                                  [--max-workspace 1073741824] [--log profiles/bench_markers.log]

Per (N, d, G), on resident inputs, HIP events around the C-ABI calls, one warm-up run, the median of --reps runs:
  moments   jamie_group_moments: time and the 4 N d bytes it must read over that time;
  rank sums jamie_group_rank_sums over all feature groups under --max-workspace, run to the end of stage 1 (key pass), 2 (chunk
            sort), 3 (merge passes) and 4 (ranking): the time of a stage is the difference of two medians, the total is the run to
            stage 4;
  yardstick jamie_feature_auroc of the same matrix against a noisy copy of itself (about half the cells positive), alternating
            with the rank sums run by run in the same process: it sorts about half the keys and ranks about half the cells with
            one pair of searches each.
On the last shape --check sampled features are recomputed on the host (`scipy.stats.rankdata`) and the integers compared.  At
--host-shape also the wall time of `JAMIE(metrics='host').rank_features` and of the whole device call from host arrays.  Prints one
line per shape and a JSON line at the end; --log writes the same lines to a file."""
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
from jamie_amd import markers as jmk  # noqa: E402

STAGES = ('key pass', 'chunk sort', 'merge passes', 'ranking')


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3


def timed(fns, reps):
    """Medians of the functions' times, run alternately: one warm-up each, then `reps` rounds of one run each."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ts[k].append(event_time(fn))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def draw(N, d, G, seed):
    """Zero-inflated log1p-like values whose rate of non-zeros is raised in group f mod G of feature f, and the group codes."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    codes = torch.randint(0, G, (N,), device='cuda', generator=g)
    marked = codes[:, None] == (torch.arange(d, device='cuda') % G)[None, :]
    X = torch.log1p(torch.floor(-3.0 * torch.log(torch.rand(N, d, device='cuda', generator=g))))
    X *= torch.rand(N, d, device='cuda', generator=g) < torch.where(marked, 0.8, 0.3)
    return X, codes.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='100000x2000x40,1000000x128x40')
    ap.add_argument('--host-shape', default='8192x128x40')
    ap.add_argument('--check', type=int, default=16)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--max-workspace', type=int, default=1 << 30)
    ap.add_argument('--log', default=None)
    a = ap.parse_args()
    nv.require_gpu()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    prop = torch.cuda.get_device_properties(0)
    say(f'device: {prop.name}, {prop.multi_processor_count} CUs; CHUNK = {jmk.CHUNK}, PIECE = {jmk.PIECE}, workspace cap '
        f'{a.max_workspace} bytes, median of {a.reps} runs after a warm-up, rank sums and feature_auroc alternating')
    shapes = [tuple(int(v) for v in s.split('x')) for s in a.shapes.split(',') if s]
    rows = []
    for si, (N, d, G) in enumerate(shapes):
        p = jmk.plan(N, d, a.max_workspace)
        X, codes = draw(N, d, G, N + d)
        lay = jmk.group_layout(codes)
        dv = {k: torch.from_numpy(lay[k]).cuda() for k in ('order', 'sorted_codes', 'seg_off', 'piece_off')}
        Y = X + 0.5 * torch.randn(N, d, device='cuda') - 0.4          # the yardstick's labels: Y > 0 on about half the cells
        thr = torch.zeros(d, device='cuda')
        R2 = torch.empty(d, G, dtype=torch.int64, device='cuda')
        tie = torch.empty(d, dtype=torch.int64, device='cuda')
        counts = torch.empty(2, d, dtype=torch.int64, device='cuda')
        sums = torch.empty(G, d, 2, dtype=torch.float64, device='cuda')
        ws = torch.empty(max(p['workspace'], nv.markers_workspace(N, d, G, 0)), dtype=torch.uint8, device='cuda')
        n_pieces = int(lay['piece_off'][-1])

        def rank(last_stage):
            for f0, dg in p['groups']:
                nv.group_rank_sums(X, dv['order'], dv['sorted_codes'], G, f0, dg, R2, tie, ws, last_stage)

        def auroc(last_stage):
            for f0, dg in p['groups']:
                nv.feature_auroc(X, Y, thr, f0, dg, counts[0], counts[1], ws, last_stage)

        t_m = timed([lambda: nv.group_moments(X, dv['order'], dv['seg_off'], dv['piece_off'], G, n_pieces, sums, ws)], a.reps)[0]
        pairs = [timed([lambda s=s: rank(s), lambda s=s: auroc(s)], a.reps) for s in (1, 2, 3, 4)]
        t_r, t_a = [q[0] for q in pairs], [q[1] for q in pairs]
        st_r = [t_r[0][0]] + [t_r[i][0] - t_r[i - 1][0] for i in (1, 2, 3)]
        st_a = [t_a[0][0]] + [t_a[i][0] - t_a[i - 1][0] for i in (1, 2, 3)]
        positives = float(counts[0].double().mean().item()) / N
        ratio = t_r[3][0] / t_a[3][0]
        r = {'N': N, 'd': d, 'G': G, 'reps': a.reps, 'groups': len(p['groups']), 'runs': p['runs'], 'merge_passes': p['passes'],
             'workspace_bytes': p['workspace'], 'pieces': n_pieces, 'moments_s': t_m[0], 'moments_s_min_max': t_m[1:],
             'moments_bytes_per_s': 4 * N * d / t_m[0], 'rank_sums_s': t_r[3][0], 'rank_sums_s_min_max': t_r[3][1:],
             'rank_sums_stage_s': dict(zip(STAGES, st_r)), 'feature_auroc_s': t_a[3][0], 'feature_auroc_s_min_max': t_a[3][1:],
             'feature_auroc_stage_s': dict(zip(STAGES, st_a)), 'feature_auroc_positive_share': positives,
             'rank_sums_over_feature_auroc': ratio}
        line = (f"N={N} d={d} G={G}: moments {t_m[0] * 1e3:.3f} ms ({t_m[1] * 1e3:.3f}-{t_m[2] * 1e3:.3f}), "
                f"{r['moments_bytes_per_s'] / 1e12:.2f} TB/s of the 4 N d bytes it reads, {n_pieces} pieces; rank sums "
                f"{t_r[3][0] * 1e3:.2f} ms ({t_r[3][1] * 1e3:.2f}-{t_r[3][2] * 1e3:.2f}) in {len(p['groups'])} group(s), {p['runs']} runs, "
                f"{p['passes']} merge passes: " + ', '.join(f'{n} {t * 1e3:.2f}' for n, t in zip(STAGES, st_r)) +
                f" ms; feature_auroc of the same matrix ({positives:.2f} of the cells positive) {t_a[3][0] * 1e3:.2f} ms "
                f"({t_a[3][1] * 1e3:.2f}-{t_a[3][2] * 1e3:.2f}): " + ', '.join(f'{n} {t * 1e3:.2f}' for n, t in zip(STAGES, st_a)) +
                f" ms; rank sums / feature_auroc = {ratio:.2f}")
        if si == len(shapes) - 1 and a.check > 0:
            from scipy.stats import rankdata
            feats = np.sort(np.random.default_rng(0).choice(d, min(a.check, d), replace=False))
            hx = X[:, feats.tolist()].cpu().numpy().astype(np.float64)
            want = np.stack([np.bincount(lay['codes'], weights=2.0 * rankdata(hx[:, k]), minlength=G) for k in range(len(feats))])
            got, got_tie = R2.cpu().numpy()[feats], tie.cpu().numpy()[feats]
            want_tie = []
            for k in range(len(feats)):
                t = np.unique(hx[:, k], return_counts=True)[1].astype(object)
                want_tie.append(int((t ** 3 - t).sum()))
            same = int(sum(np.array_equal(got[k], np.rint(want[k]).astype(np.int64)) and int(got_tie[k]) == want_tie[k]
                           for k in range(len(feats))))
            r['cross_check'] = {'features': len(feats), 'equal': same}
            line += f'; cross-check against the host: rank sums and tie term equal on {same} of {len(feats)} sampled features'
        rows.append(r)
        say(line)
        del X, Y, ws, R2, tie, counts, sums, thr, dv
        torch.cuda.empty_cache()
    host = None
    if a.host_shape:
        from jamie_amd import JAMIE
        N, d, G = (int(v) for v in a.host_shape.split('x'))
        X, codes = draw(N, d, G, N + d)
        hx = X.cpu().numpy()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            ref = JAMIE(metrics='host').rank_features(hx, codes)
        t_host = time.perf_counter() - t0
        jmk.rank_features(hx, codes)                                   # warm-up
        t0 = time.perf_counter()
        out = jmk.rank_features(hx, codes)
        t_dev = time.perf_counter() - t0
        equal = bool(np.array_equal(out['rank_sum2'], ref['rank_sum2']) and np.array_equal(out['tie_term'], ref['tie_term'])
                     and out['z'].tobytes() == ref['z'].tobytes())
        host = {'N': N, 'd': d, 'G': G, 'host_rank_features_s': t_host, 'device_rank_features_wall_s': t_dev, 'integers_and_z_equal': equal}
        say(f"N={N} d={d} G={G}: host rank_features {t_host:.2f} s wall, the device call from host arrays {t_dev * 1e3:.1f} ms wall; "
            f"rank sums, tie term and z equal: {equal}")
    say(json.dumps({'bench_markers': rows, 'host': host, 'imputation_chunk': ji.CHUNK}))
    if a.log:
        with open(a.log, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

"""Louvain communities on the device: one level-0 sweep and the whole call, on resident inputs.

    python tools/bench_louvain.py [--cases 200000x32,1000000x32] [--reps 5] [--log PATH]

Without --child the tool only starts one fresh process per case, each under its own time limit, and stops at the first step that
fails; it does not touch the GPU itself.  A child (--child NxL) builds the fuzzy graph of 40 overlapping blobs (one connected
graph) and measures, with HIP events around the calls, median of --reps rounds after a warm-up round:

    alternating in the same process: the first sweep of level 0 from singletons (its 8 sub-sweeps: 8 `jamie_louvain_move` and 8
        `jamie_louvain_apply` calls, no read-back in between) and one `jamie_graph_cheb_step` (B = 16, with `prev`) over the same CSR
        arrays -- a pass that reads every stored entry once, as a sub-sweep reads an eighth of them
    then, by the wall clock: `louvain.communities` on the resident graph, and a whole `louvain.louvain` call on the resident cells
        (neighbour lists and graph included)

No time is fixed in advance; what a run did not measure is written as such.  Prints one line per figure, a JSON line at the end,
and appends both to --log."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def child_case(N, L, a, say):
    import torch
    from bench_spectral import overlapping
    from bench_umap import event_time
    from jamie_amd import louvain as jlv
    from jamie_amd import spectral as js
    nn = a.n_neighbors
    reps = a.reps if N < 500000 else 3
    X = overlapping(N, L, N + L)
    G = js.build_graph(X, nn)
    nnz = int(G.col.numel())
    lens = G.rowptr[1:] - G.rowptr[:-1]
    LG = jlv.level_graph(G)
    plan = LG.plan()
    bins = plan['counts'].sum(axis=0).tolist()
    scale, _ = js.normalised_operator(G, False)
    g = torch.Generator(device='cuda').manual_seed(16)
    Xb, P, O = (torch.randn(N, 16, dtype=torch.float64, device='cuda', generator=g) for _ in range(3))
    state = jlv.singletons(LG)

    def run_sweep():
        for s in range(jlv.CLASSES):
            jlv.move(LG, state, s, 1.0)
            jlv.apply(LG, state, s)

    def run_step():
        js.cheb_step(G, scale, Xb, P, O, 1.1, -0.2, 0.3)
    run_sweep()
    run_step()
    torch.cuda.synchronize()
    tw, ts, moved = [], [], []
    for _ in range(reps):
        state = jlv.singletons(LG)
        torch.cuda.synchronize()
        tw.append(event_time(run_sweep))
        moved.append(int(state.moved.item()))
        ts.append(event_time(run_step))
    t_sweep, t_step = statistics.median(tw), statistics.median(ts)
    say(f"N={N}, L={L}, n_neighbors={nn}: nnz {nnz}, longest row {int(lens.max().item())}, rows per bin (short, long, global) {bins}; "
        f"first sweep of level 0 (8 sub-sweeps, {moved[0]} nodes moved) {t_sweep * 1e3:.3f} ms ({min(tw) * 1e3:.3f}-{max(tw) * 1e3:.3f}); "
        f"cheb_step B=16 over the same CSR arrays {t_step * 1e3:.3f} ms ({min(ts) * 1e3:.3f}-{max(ts) * 1e3:.3f}): sweep / step "
        f"{t_sweep / t_step:.2f}")
    out = {'pooled': N, 'L': L, 'n_neighbors': nn, 'reps': reps, 'nnz': nnz, 'rows_per_bin': bins, 'sweep_s': t_sweep,
           'sweep_s_min_max': (min(tw), max(tw)), 'moved_first_sweep': moved, 'cheb_step_b16_s': t_step,
           'cheb_step_s_min_max': (min(ts), max(ts)), 'sweep_over_step': t_sweep / t_step}
    del Xb, P, O
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = jlv.communities(G)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    again = jlv.communities(G)
    same = bool((again['clusters'] == res['clusters']).all()) and again['modularity'] == res['modularity']
    say(f"communities on the resident graph, {N} cells: {wall:.2f} s wall, {len(res['sizes'])} clusters, modularity {res['modularity']:.6f}, "
        f"levels (nodes, sweeps) {[(lv['nodes'], lv['sweeps']) for lv in res['levels']]}; a second run gives the same bits: {same}")
    out['communities'] = {'wall_s': wall, 'n_clusters': len(res['sizes']), 'modularity': res['modularity'], 'repeatable': same,
                          'levels': [(lv['nodes'], lv['communities'], lv['sweeps']) for lv in res['levels']]}
    del G, LG, state
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    full = jlv.louvain([X], n_neighbors=nn)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    say(f"louvain, {N} cells, L={L}, n_neighbors={nn} (neighbour lists and graph included): {wall:.2f} s wall, {full['n_clusters']} "
        f"clusters, modularity {full['modularity']:.6f}")
    out['louvain'] = {'wall_s': wall, 'n_clusters': full['n_clusters'], 'modularity': full['modularity']}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='200000x32,1000000x32', help='pooled cells x L')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--n-neighbors', type=int, default=15)
    ap.add_argument('--limit', type=int, default=420, help='seconds a child may take')
    ap.add_argument('--child', default=None, help='(internal) NxL')
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'bench_louvain.log'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    if a.child is None:
        open(a.log, 'w').close()
        base = [sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), '--n-neighbors', str(a.n_neighbors), '--log', a.log]
        for step in a.cases.split(','):                      # one fresh process per case, each under its own limit; stop at a failure
            rc = subprocess.run(base + ['--child', step], timeout=a.limit).returncode
            if rc != 0:
                sys.exit(f'bench_louvain: case {step} ended with status {rc}; nothing further was started')
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    import torch
    from jamie_amd import _native as nv
    nv.require_gpu()
    prop = torch.cuda.get_device_properties(0)
    say(f'device: {prop.name}, {prop.multi_processor_count} CUs')
    N, L = (int(v) for v in a.child.split('x'))
    out = {'bench_louvain': child_case(N, L, a, say)}
    say(json.dumps(out))
    with open(a.log, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

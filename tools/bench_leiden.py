"""Leiden communities on the device: one refinement pass of level 0 and the whole call, beside Louvain's, on resident inputs.

    python tools/bench_leiden.py [--cases 200000x32,1000000x32] [--reps 5] [--log PATH]

Without --child the tool only starts one fresh process per case, each under its own time limit, and stops at the first step that
fails; it does not touch the GPU itself.  A child (--child NxL) builds the fuzzy graph of 40 overlapping blobs (one connected
graph) and measures, with HIP events around the calls, median of --reps rounds after a warm-up round (3 rounds from 500 000 cells):

    alternating in the same process over the same arrays: one refinement pass of level 0 inside the communities of its move phase
        (8 sub-sweeps: 8 device copies of ref, 8 `jamie_leiden_cut`, 8 `jamie_leiden_refine` and 8 `jamie_leiden_apply` calls, no
        read-back in between) and the first Louvain sweep of level 0 from singletons (8 `jamie_louvain_move` and 8
        `jamie_louvain_apply` calls) as the yardstick; the pass again with the cut calls left out and with only the cut calls
        (what the rest and the cut table cost: the results of the first are not the definition's)
    then, by the wall clock: `leiden.communities` and `louvain.communities` on the resident graph, and a whole `leiden.leiden`
        and `louvain.louvain` call on the resident cells (neighbour lists and graph included)

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
    from jamie_amd import leiden as jld
    from jamie_amd import louvain as jlv
    from jamie_amd import spectral as js
    nn = a.n_neighbors
    reps = a.reps if N < 500000 else 3
    X = overlapping(N, L, N + L)
    G = js.build_graph(X, nn)
    nnz = int(G.col.numel())
    LG = jlv.level_graph(G)
    bins = LG.plan()['counts'].sum(axis=0).tolist()
    moved, history = jlv.run_level(LG, 1.0, 32)
    n_comm = int((moved.size > 0).sum().item())
    R = jld.start(LG)
    state = jlv.singletons(LG)

    def run_pass(cut=True, rest=True):
        for s in range(jlv.CLASSES):
            if rest:
                R.target.copy_(R.ref)
            if cut:
                jld.cut_table(LG, moved.comm, R)
            if rest:
                jld.refine(LG, moved, R, s, 1.0)
                jld.apply(LG, R, s)

    def run_sweep():
        for s in range(jlv.CLASSES):
            jlv.move(LG, state, s, 1.0)
            jlv.apply(LG, state, s)
    run_pass()
    run_sweep()
    torch.cuda.synchronize()
    tp, tw, tr, tc, counts = [], [], [], [], []
    for _ in range(reps):
        R = jld.start(LG)
        state = jlv.singletons(LG)
        torch.cuda.synchronize()
        tp.append(event_time(run_pass))
        counts.append(R.counts.tolist())
        tw.append(event_time(run_sweep))
        R = jld.start(LG)
        torch.cuda.synchronize()
        tr.append(event_time(lambda: run_pass(cut=False)))
        R = jld.start(LG)
        torch.cuda.synchronize()
        tc.append(event_time(lambda: run_pass(rest=False)))
    if int(R.flag.item()) or int(state.flag.item()):
        raise RuntimeError('bench_leiden: a row did not fit its bin')
    t_pass, t_sweep, t_rest, t_cut = (statistics.median(t) for t in (tp, tw, tr, tc))
    say(f"N={N}, L={L}, n_neighbors={nn}: nnz {nnz}, rows per bin (short, long, global) {bins}; move phase of level 0: {len(history)} "
        f"sweeps, {n_comm} communities; one refinement pass (8 sub-sweeps, {counts[0][0]} merged, {counts[0][1]} cancelled) "
        f"{t_pass * 1e3:.3f} ms ({min(tp) * 1e3:.3f}-{max(tp) * 1e3:.3f}); first Louvain sweep of level 0 {t_sweep * 1e3:.3f} ms "
        f"({min(tw) * 1e3:.3f}-{max(tw) * 1e3:.3f}): pass / sweep {t_pass / t_sweep:.2f}; the pass without its 8 cut calls "
        f"{t_rest * 1e3:.3f} ms, its 8 cut calls alone {t_cut * 1e3:.3f} ms")
    out = {'pooled': N, 'L': L, 'n_neighbors': nn, 'reps': reps, 'nnz': nnz, 'rows_per_bin': bins, 'communities_level0': n_comm,
           'pass_s': t_pass, 'pass_s_min_max': (min(tp), max(tp)), 'merged_cancelled': counts, 'sweep_s': t_sweep,
           'sweep_s_min_max': (min(tw), max(tw)), 'pass_over_sweep': t_pass / t_sweep, 'pass_without_cut_s': t_rest, 'cut_calls_s': t_cut}
    del R, state, moved
    for tag, mod in (('leiden', jld), ('louvain', jlv)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = mod.communities(G)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        again = mod.communities(G)
        same = bool((again['clusters'] == res['clusters']).all()) and again['modularity'] == res['modularity']
        say(f"{tag}.communities on the resident graph, {N} cells: {wall:.2f} s wall, {len(res['sizes'])} clusters, modularity "
            f"{res['modularity']:.6f}, stop {res.get('stop')}, levels (nodes, sweeps) {[(lv['nodes'], lv['sweeps']) for lv in res['levels']]}; a "
            f"second run gives the same bits: {same}")
        out[f'{tag}_communities'] = {'wall_s': wall, 'n_clusters': len(res['sizes']), 'modularity': res['modularity'], 'repeatable': same,
                                     'stop': res.get('stop'), 'levels': [(lv['nodes'], lv['communities'], lv['sweeps']) for lv in res['levels']]}
    del G, LG
    for tag, call in (('leiden', jld.leiden), ('louvain', jlv.louvain)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        full = call([X], n_neighbors=nn)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        say(f"{tag}, {N} cells, L={L}, n_neighbors={nn} (neighbour lists and graph included): {wall:.2f} s wall, {full['n_clusters']} "
            f"clusters over {len(full['levels'])} levels, modularity {full['modularity']:.6f}")
        out[tag] = {'wall_s': wall, 'n_clusters': full['n_clusters'], 'levels': len(full['levels']), 'modularity': full['modularity']}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='200000x32,1000000x32', help='pooled cells x L')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--n-neighbors', type=int, default=15)
    ap.add_argument('--limit', type=int, default=420, help='seconds a child may take')
    ap.add_argument('--child', default=None, help='(internal) NxL')
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'bench_leiden.log'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    if a.child is None:
        open(a.log, 'w').close()
        base = [sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), '--n-neighbors', str(a.n_neighbors), '--log', a.log]
        for step in a.cases.split(','):                      # one fresh process per case, each under its own limit; stop at a failure
            rc = subprocess.run(base + ['--child', step], timeout=a.limit).returncode
            if rc != 0:
                sys.exit(f'bench_leiden: case {step} ended with status {rc}; nothing further was started')
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
    out = {'bench_leiden': child_case(N, L, a, say)}
    say(json.dumps(out))
    with open(a.log, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

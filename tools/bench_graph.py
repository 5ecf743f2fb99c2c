"""Graph structure on the device: the hook, the jump and the kBET kernel beside existing passes over the same arrays, the whole
`components` run and the whole `graph_metrics` call, on resident inputs.

    python tools/bench_graph.py [--cases 200000x32,1000000x32] [--reps 5] [--log PATH]

Without --child the tool only starts one fresh process per case, each under its own time limit, and stops at the first step that
fails; it does not touch the GPU itself.  A child (--child NxL) builds the neighbour lists and the fuzzy graph of 40 overlapping
blobs (one connected graph) and measures, with HIP events around the calls, median of --reps rounds (3 from 500 000 cells on)
after a warm-up round:

    alternating in the same process, over the same CSR arrays: the first hook launch (root = the node ids: every entry differs,
        the launch with the most atomics), the hook of the second round, the hook of the last round (no entry differs), the first
        sweep of Louvain's level 0 from singletons (8 `jamie_louvain_move` and 8 `jamie_louvain_apply` calls) and one
        `jamie_graph_cheb_step` (B = 16, with `prev`)
    a jump pass on the array the first hook leaves, beside a device copy of n int32
    `jamie_kbet_stat` (2 modalities) beside `jamie_lisi` (1 set, perplexity 4) on the same lists
    then, by the wall clock: `components` on the resident graph with its rounds and jumps, and a whole `graph_metrics` call on two
        resident embeddings with labels (neighbour lists and graph included)

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
    import numpy as np
    import torch
    from bench_spectral import overlapping
    from bench_umap import event_time
    from jamie_amd import _native as nv
    from jamie_amd import graph as jgr
    from jamie_amd import louvain as jlv
    from jamie_amd import spectral as js
    from jamie_amd import umap as jum
    from jamie_amd.neighbors import self_knn
    nn = a.n_neighbors
    reps = a.reps if N < 500000 else 3
    X = overlapping(N, L, N + L)
    idx, dist = self_knn(X, nn - 1)
    W, _, _, _ = jum.smooth_knn(idx, dist, nn)
    G = jum.fuzzy_graph(idx, W)
    del W
    nnz = int(G.col.numel())
    lens = G.rowptr[1:] - G.rowptr[:-1]
    trace = []
    label, rounds, jumps = jgr.components(G, trace=trace)
    roots = [t for tag, t in trace if tag == 'root']
    first_parent = trace[0][1]
    del trace
    ident = torch.arange(N, dtype=torch.int32, device='cuda')
    inputs = {'first': ident, 'second': roots[0] if roots else ident, 'last': label}
    differ = {}
    row = torch.repeat_interleave(torch.arange(N, device='cuda'), lens)
    for k, r in inputs.items():
        differ[k] = int((r[row] != r[G.col.long()]).sum().item())
    del row
    parent, spare = torch.empty_like(ident), torch.empty_like(ident)
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    LG = jlv.level_graph(G)
    LG.plan()
    scale, _ = js.normalised_operator(G, False)
    g = torch.Generator(device='cuda').manual_seed(16)
    Xb, P, O = (torch.randn(N, 16, dtype=torch.float64, device='cuda', generator=g) for _ in range(3))
    state = jlv.singletons(LG)

    def run_hook(which):
        def fn():
            nv.graph_hook(G.rowptr, G.col, None, inputs[which], parent, flag)
        return fn

    def run_sweep():
        for s in range(jlv.CLASSES):
            jlv.move(LG, state, s, 1.0)
            jlv.apply(LG, state, s)

    def run_step():
        js.cheb_step(G, scale, Xb, P, O, 1.1, -0.2, 0.3)

    def run_jump():
        nv.graph_jump(first_parent, spare, flag)

    def run_copy():
        spare.copy_(first_parent)
    parent.copy_(ident)
    for fn in (run_hook('first'), run_sweep, run_step, run_jump, run_copy):
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in ('first', 'second', 'last', 'sweep', 'step', 'jump', 'copy')}
    for _ in range(reps):
        for which in ('first', 'second', 'last'):
            parent.copy_(inputs[which])
            torch.cuda.synchronize()
            t[which].append(event_time(run_hook(which)))
        state = jlv.singletons(LG)
        torch.cuda.synchronize()
        t['sweep'].append(event_time(run_sweep))
        t['step'].append(event_time(run_step))
        t['jump'].append(event_time(run_jump))
        t['copy'].append(event_time(run_copy))
    med = {k: statistics.median(v) for k, v in t.items()}

    def span(k):
        return f'{med[k] * 1e3:.3f} ms ({min(t[k]) * 1e3:.3f}-{max(t[k]) * 1e3:.3f})'
    say(f"N={N}, L={L}, n_neighbors={nn}: nnz {nnz}, longest row {int(lens.max().item())}; hook launches over the CSR arrays: first "
        f"({differ['first']} entries differ) {span('first')}, second round ({differ['second']} differ) {span('second')}, last round "
        f"({differ['last']} differ) {span('last')}; first Louvain sweep of level 0 (8 sub-sweeps) {span('sweep')}; cheb_step B=16 "
        f"{span('step')}: first hook / sweep {med['first'] / med['sweep']:.2f}, first hook / step {med['first'] / med['step']:.2f}, last "
        f"hook / step {med['last'] / med['step']:.2f}")
    say(f"jump pass over {N} nodes {span('jump')}; device copy of {N} int32 {span('copy')}: jump / copy {med['jump'] / med['copy']:.2f}")
    out = {'pooled': N, 'L': L, 'n_neighbors': nn, 'reps': reps, 'nnz': nnz, 'entries_that_differ': differ,
           'seconds': med, 'seconds_min_max': {k: (min(v), max(v)) for k, v in t.items()},
           'first_hook_over_sweep': med['first'] / med['sweep'], 'first_hook_over_step': med['first'] / med['step'],
           'jump_over_copy': med['jump'] / med['copy']}
    del Xb, P, O, LG, state, scale
    # kBET beside LISI on the same lists
    codes = (torch.arange(N, device='cuda') % 2).to(torch.int32)
    shares = torch.tensor([[0.5, 0.5]], dtype=torch.float64, device='cuda')
    stat = torch.empty(N, dtype=torch.float64, device='cuda')
    df = torch.empty(N, dtype=torch.int32, device='cuda')
    lisi = torch.empty(1, N, dtype=torch.float64, device='cuda')
    codes2 = codes.view(1, N)

    def run_kbet():
        nv.kbet_stat(idx, codes, shares, None, stat, df, None)

    def run_lisi():
        nv.lisi(idx, dist, codes2, 4.0, lisi, None)
    run_kbet()
    run_lisi()
    torch.cuda.synchronize()
    tk, tl = [], []
    for _ in range(reps):
        tk.append(event_time(run_kbet))
        tl.append(event_time(run_lisi))
    mk, ml = statistics.median(tk), statistics.median(tl)
    say(f"jamie_kbet_stat, {N} cells x {nn - 1} neighbours, 2 categories {mk * 1e3:.3f} ms ({min(tk) * 1e3:.3f}-{max(tk) * 1e3:.3f}); "
        f"jamie_lisi on the same lists (1 set, perplexity 4) {ml * 1e3:.3f} ms ({min(tl) * 1e3:.3f}-{max(tl) * 1e3:.3f}): kbet / lisi "
        f"{mk / ml:.2f}")
    out.update(kbet_s=mk, kbet_s_min_max=(min(tk), max(tk)), lisi_s=ml, lisi_s_min_max=(min(tl), max(tl)), kbet_over_lisi=mk / ml)
    del idx, dist, stat, df, lisi
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    again, r2, j2 = jgr.components(G)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    same = bool(torch.equal(again, label)) and (r2, j2) == (rounds, jumps)
    say(f"components on the resident graph, {N} cells: {wall * 1e3:.2f} ms wall, {rounds} rounds, {jumps} jumps, "
        f"{int(torch.unique(label).numel())} components; a second run gives the same bits: {same}")
    out['components'] = {'wall_s': wall, 'rounds': rounds, 'jumps': jumps, 'n_components': int(torch.unique(label).numel()),
                         'repeatable': same}
    del G, label, again, roots, inputs, first_parent
    half = N // 2
    labels = np.arange(N) % 7
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    full = jgr.graph_metrics([X[:half], X[half:]], [labels[:half], labels[half:]], n_neighbors=nn)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    say(f"graph_metrics, {N} cells in 2 embeddings, 7 labels, L={L}, n_neighbors={nn} (neighbour lists and graph included): {wall:.2f} s "
        f"wall, {full['n_components']} components, graph connectivity {full['graph_connectivity']:.4f}, kBET rejection "
        f"{full['kbet_rejection']:.4f}")
    out['graph_metrics'] = {'wall_s': wall, 'n_components': full['n_components'], 'graph_connectivity': full['graph_connectivity'],
                            'kbet_rejection': full['kbet_rejection'], 'rounds': full['rounds'], 'jumps': full['jumps']}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='200000x32,1000000x32', help='pooled cells x L')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--n-neighbors', type=int, default=15)
    ap.add_argument('--limit', type=int, default=420, help='seconds a child may take')
    ap.add_argument('--child', default=None, help='(internal) NxL')
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'bench_graph.log'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    if a.child is None:
        open(a.log, 'w').close()
        base = [sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), '--n-neighbors', str(a.n_neighbors), '--log', a.log]
        for step in a.cases.split(','):                      # one fresh process per case, each under its own limit; stop at a failure
            rc = subprocess.run(base + ['--child', step], timeout=a.limit).returncode
            if rc != 0:
                sys.exit(f'bench_graph: case {step} ended with status {rc}; nothing further was started')
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
    out = {'bench_graph': child_case(N, L, a, say)}
    say(json.dumps(out))
    with open(a.log, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

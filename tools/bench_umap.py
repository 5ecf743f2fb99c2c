"""UMAP on the device: the smooth-kNN solve, the graph build, the epochs and the whole call, on resident inputs.

    python tools/bench_umap.py [--cases 200000x32,1000000x32] [--wall-cells 200000] [--log PATH]

Without --child the tool only starts one fresh process per case (and one for the whole-call timing), each under its own time limit,
and stops at the first that fails; it does not touch the GPU itself.  A child (--child NxL) measures with HIP events around the
C-ABI calls, median of --reps rounds after a warm-up round:

    the smooth-kNN solve, the graph build (wall: it holds a sort), the schedule
    a whole run of n_epochs epochs enqueued back to back from a fresh schedule and a uniform layout on [0, 10]^2: the mean epoch,
        firings/s, and bytes/s counting per entry `next` and `eps` (8), per firing the write of `next`, the column and y_j (16) and
        8 per negative draw, per row the two offsets, y_in and y_out (32); beside a device copy of the same number of bytes
    alternating in the same process: one epoch at the middle of the schedule, `jamie_tsne_step`'s attraction pass over the same CSR
        arrays (the same rows walked by one wave each: the yardstick of an epoch), and one whole t-SNE iteration at the same N

Prints one line per case, a JSON line at the end, and appends both to --log."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_time(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3


def blobs(N, L, seed, n_blobs=40):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    lab = torch.randint(0, n_blobs, (N,), device='cuda', generator=g)
    return 2.0 * torch.randn(n_blobs, L, device='cuda', generator=g)[lab] + torch.randn(N, L, device='cuda', generator=g)


def child_case(N, L, a, say):
    import numpy as np
    import torch
    from jamie_amd import _native as nv
    from jamie_amd import tsne as jt
    from jamie_amd import umap as ju
    from jamie_amd.neighbors import self_knn
    nn, neg = a.n_neighbors, 5
    reps = a.reps if N < 500000 else 3
    n_epochs = ju.default_epochs(N)
    ca, cb = ju.find_ab(1.0, 0.1)
    X = blobs(N, L, N + L)
    idx, dist = self_knn(X, nn - 1)
    del X
    K = nn - 1
    W = torch.empty(N, K, dtype=torch.float32, device='cuda')
    rho = torch.empty(N, dtype=torch.float64, device='cuda')
    sigma = torch.empty(N, dtype=torch.float64, device='cuda')
    tries = torch.empty(N, dtype=torch.int32, device='cuda')

    def run_smooth():
        nv.umap_smooth_knn(dist, nn, ju.smooth_target(nn), W, rho, sigma, tries)
    run_smooth()
    t_smooth = statistics.median([event_time(run_smooth) for _ in range(reps)])
    ju.fuzzy_graph(idx, W)
    tg = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        G = ju.fuzzy_graph(idx, W)
        torch.cuda.synchronize()
        tg.append(time.perf_counter() - t0)
    t_graph = statistics.median(tg)
    nnz = int(G.col.numel())
    longest = int((G.rowptr[1:] - G.rowptr[:-1]).max().item())
    del idx, dist, W
    eps, nxt0 = ju.edge_schedule(G, n_epochs)
    pruned = int(torch.isinf(eps).sum().item())
    Y0 = torch.from_numpy(np.random.default_rng(1).uniform(0, 10, (N, 2)).astype(np.float32)).cuda()
    total = torch.zeros(N, dtype=torch.int64, device='cuda')
    ju.optimize(G, Y0, eps, nxt0.clone(), n_epochs, 1.0, ca, cb, seed=0, count=2)          # warm-up (and the graph's column check)
    runs = []
    for _ in range(reps):
        nxt = nxt0.clone()
        total.zero_()
        runs.append(event_time(lambda: ju.optimize(G, Y0, eps, nxt, n_epochs, 1.0, ca, cb, 1.0, neg, 0, fired_total=total)))
    t_run = statistics.median(runs)
    n_fired = int(total.sum().item())
    bytes_run = n_epochs * (8 * nnz + 32 * N) + n_fired * (16 + 8 * neg)
    src = torch.empty(bytes_run // n_epochs // 2, dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(src)
    dst.copy_(src)
    t_copy = statistics.median([event_time(lambda: dst.copy_(src)) for _ in range(reps)])
    del src, dst
    # alternating: one epoch at the middle of the schedule, the attraction pass of t-SNE over the same rows, one t-SNE iteration
    mid = n_epochs // 2
    nxt_mid = nxt0.clone()
    Ymid = ju.optimize(G, Y0, eps, nxt_mid, n_epochs, 1.0, ca, cb, seed=0, count=mid)
    Yout = torch.empty_like(Ymid)
    nxt_work = nxt_mid.clone()
    buf = jt._Gradient(N, Ymid.device, 0)
    buf.R.zero_()
    buf.Z.fill_(1.0)
    grad = torch.empty(N, 2, dtype=torch.float32, device='cuda')
    u = torch.zeros_like(Ymid)
    gain = torch.ones_like(Ymid)
    Yt = Ymid.clone()

    def run_epoch():
        nxt_work.copy_(nxt_mid)

    def run_epoch_timed():
        ju.epoch(G, Ymid, Yout, eps, nxt_work, mid, ju.alpha_of(1.0, mid, n_epochs), ca, cb, 1.0, neg, 0)

    def run_attract():
        nv.tsne_step(G.rowptr, G.col, G.val, Yt, buf.R, buf.Z, 1.0, 0.0, 1.0, None, None, False, buf.ws_step, grad=grad)

    def run_tsne_iter():                                    # (lr = 1e-30 keeps the layout where it is)
        nv.tsne_repulsion(Yt, buf.R, buf.z, buf.Z, buf.ws_rep, 0)
        nv.tsne_step(G.rowptr, G.col, G.val, Yt, buf.R, buf.Z, 1.0, 0.8, 1e-30, u, gain, True, buf.ws_step)
    for warm in (run_epoch, run_epoch_timed, run_attract, run_tsne_iter):
        warm()
    torch.cuda.synchronize()
    te, ta, tt = [], [], []
    for _ in range(reps):
        run_epoch()
        te.append(event_time(run_epoch_timed))
        ta.append(event_time(run_attract))
        tt.append(event_time(run_tsne_iter))
    t_epoch, t_att, t_tsne = statistics.median(te), statistics.median(ta), statistics.median(tt)
    fired_mid = int((nxt_mid <= float(mid)).sum().item())
    r = {'pooled': N, 'L': L, 'n_neighbors': nn, 'n_epochs': n_epochs, 'reps': reps, 'nnz': nnz, 'longest_row': longest,
         'never_fire': pruned, 'smooth_knn_s': t_smooth, 'tries_max': int(tries.max().item()), 'graph_wall_s': t_graph,
         'run_s': t_run, 'run_s_min_max': (min(runs), max(runs)), 'epoch_mean_s': t_run / n_epochs, 'n_fired': n_fired,
         'firings_per_s': n_fired / t_run, 'bytes_per_epoch': bytes_run / n_epochs, 'bytes_per_s': bytes_run / t_run,
         'copy_same_bytes_s': t_copy, 'copy_bytes_per_s': bytes_run / n_epochs / t_copy, 'epoch_mid_s': t_epoch,
         'epoch_mid_s_min_max': (min(te), max(te)), 'epoch_mid_firings': fired_mid, 'tsne_attraction_s': t_att,
         'tsne_attraction_s_min_max': (min(ta), max(ta)), 'tsne_iteration_s': t_tsne, 'epoch_over_attraction': t_epoch / t_att,
         'tsne_iteration_over_epoch_mean': t_tsne / (t_run / n_epochs)}
    say(f"N={N}, L={L}, n_neighbors={nn}: smooth-kNN solve {t_smooth * 1e3:.3f} ms (at most {r['tries_max']} tries); graph build "
        f"{t_graph * 1e3:.1f} ms wall, nnz {nnz}, longest row {longest}, {pruned} entries never fire; {n_epochs} epochs "
        f"{t_run * 1e3:.1f} ms ({min(runs) * 1e3:.1f}-{max(runs) * 1e3:.1f}): mean epoch {t_run / n_epochs * 1e3:.3f} ms, {n_fired} firings, "
        f"{n_fired / t_run / 1e9:.2f} G firings/s, {bytes_run / t_run / 1e12:.3f} TB/s of {bytes_run / n_epochs / 1e6:.1f} MB per epoch; a "
        f"device copy of the same bytes {t_copy * 1e3:.3f} ms ({r['copy_bytes_per_s'] / 1e12:.2f} TB/s); epoch {mid} alone "
        f"{t_epoch * 1e3:.3f} ms ({min(te) * 1e3:.3f}-{max(te) * 1e3:.3f}, {fired_mid} firings); t-SNE attraction pass over the same "
        f"rows {t_att * 1e3:.3f} ms ({min(ta) * 1e3:.3f}-{max(ta) * 1e3:.3f}); epoch / attraction {t_epoch / t_att:.2f}; one t-SNE "
        f"iteration {t_tsne * 1e3:.3f} ms: {r['tsne_iteration_over_epoch_mean']:.1f} x the mean epoch")
    return r


def child_wall(N, a, say):
    import torch
    from jamie_amd import umap as ju
    X = blobs(N, 32, 7)
    ju.umap([X[:4096]], n_epochs=2)                         # (the library is loaded, the allocator is warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = ju.umap([X], n_neighbors=a.n_neighbors)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    say(f"umap, {N} cells, L=32, n_neighbors={a.n_neighbors}, {out['n_epochs']} epochs, init 'pca': {wall:.2f} s wall, {out['n_edges']} "
        f"edges, {out['n_fired']} firings")
    return {'wall_cells': N, 'L': 32, 'n_epochs': out['n_epochs'], 'wall_s': wall, 'n_edges': out['n_edges'], 'n_fired': out['n_fired']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='200000x32,1000000x32', help='pooled cells x L')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--n-neighbors', type=int, default=15)
    ap.add_argument('--wall-cells', type=int, default=200000, help='cells of the whole-call timing (0: skip)')
    ap.add_argument('--limit', type=int, default=240, help='seconds a child may take')
    ap.add_argument('--child', default=None, help='(internal) NxL, or wallN')
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'bench_umap.log'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    if a.child is None:
        open(a.log, 'w').close()
        steps = a.cases.split(',') + ([f'wall{a.wall_cells}'] if a.wall_cells > 0 else [])
        for step in steps:                                  # one fresh process per step, each under its own limit; stop at a failure
            cmd = [sys.executable, os.path.abspath(__file__), '--child', step, '--reps', str(a.reps), '--n-neighbors', str(a.n_neighbors),
                   '--log', a.log]
            rc = subprocess.run(cmd, timeout=a.limit).returncode
            if rc != 0:
                sys.exit(f'bench_umap: step {step} ended with status {rc}; nothing further was started')
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
    if a.child.startswith('wall'):
        out = {'umap_wall': child_wall(int(a.child[4:]), a, say)}
    else:
        N, L = (int(v) for v in a.child.split('x'))
        out = {'bench_umap': child_case(N, L, a, say)}
    say(json.dumps(out))
    with open(a.log, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

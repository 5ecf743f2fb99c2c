"""t-SNE on the device: the all-pairs repulsion pass, a whole iteration, the affinity solve and the build of P, on resident inputs.

    python tools/bench_tsne.py [--cases 200000x32,1000000x32,200000x64] [--wall-cells 200000] [--host-cells 8192] [--log PATH]

Per (pooled N, L): HIP events around the C-ABI calls, median of --reps rounds (3 at 10^6 cells) after one warm-up round.
`cross_knn(Y, Y, 1)` on the same 2-feature points, the cheapest walker of that pair space the library had before, alternates with
the repulsion pass in the same process.  The layout timed is a spread-out one (gaussian, sd 30).  Reported: pairs/s of the
repulsion pass (N^2 pairs) against the fp32 VALU issue ceiling in two accountings.  From the kernel's disassembly the 8-column x
4-row block of the full-tile loop is 197 VALU instructions for 32 pairs (VALU_PER_PAIR): the first figure counts every instruction
as one issue slot.  32 of them are v_rcp_f32 and 160 are packed fp32 (v_pk_fma_f32, v_pk_add_f32, v_pk_mul_f32: two lanes' worth
each); the second figure weights each of those as two slots (SLOTS_PER_PAIR), which is an ASSUMPTION about the issue cost of these
instructions, not something this tool measures.  One whole iteration is timed twice: alone between two events, and as the mean of
--batch iterations enqueued back to back between two events (what a run does).  Then the wall time of `tsne` for --wall-iters
iterations, and for context sklearn's Barnes-Hut TSNE on --host-cells cells.  Prints one line per case, a JSON line at the end, and writes both to --log."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jamie_amd import _native as nv  # noqa: E402
from jamie_amd import tsne as jt  # noqa: E402
from jamie_amd.neighbors import self_knn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALU_PER_PAIR = 197 / 32
SLOTS_PER_PAIR = (5 + 2 * 32 + 2 * 160) / 32          # assumed: a v_rcp_f32 and a packed fp32 instruction cost two plain slots each
ISSUE = 256 * 4 * 32 * 2.4e9          # lane-instructions/s: 256 CUs x 4 SIMDs x 32 lanes at 2.4 GHz (DESIGN.md §10 counts two per pair-feature)


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3


def blobs(N, L, seed, n_blobs=40):
    g = torch.Generator(device='cuda').manual_seed(seed)
    lab = torch.randint(0, n_blobs, (N,), device='cuda', generator=g)
    return 2.0 * torch.randn(n_blobs, L, device='cuda', generator=g)[lab] + torch.randn(N, L, device='cuda', generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='200000x32,1000000x32,200000x64', help='pooled cells x L')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=50, help='iterations enqueued back to back for the sustained figure')
    ap.add_argument('--perplexity', type=float, default=30.0)
    ap.add_argument('--wall-cells', type=int, default=200000, help='cells of the whole-run timing (0: skip)')
    ap.add_argument('--wall-iters', type=int, default=1000)
    ap.add_argument('--host-cells', type=int, default=8192, help='cells of the sklearn TSNE timing (0: skip)')
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'bench_tsne.log'))
    a = ap.parse_args()
    nv.require_gpu()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    say(f'device: {prop.name}, {prop.multi_processor_count} CUs')
    rows = []
    for case in a.cases.split(','):
        N, L = (int(v) for v in case.split('x'))
        K = int(3 * a.perplexity)
        reps = a.reps if N < 500000 else 3
        X = blobs(N, L, N + L)
        idx, dist = self_knn(X, K)
        del X
        C = torch.empty(N, K, dtype=torch.float32, device='cuda')
        beta = torch.empty(N, dtype=torch.float64, device='cuda')
        tries = torch.empty(N, dtype=torch.int32, device='cuda')

        def run_aff():
            nv.tsne_affinities(dist, a.perplexity, C, beta, tries)
        run_aff()
        t_aff = statistics.median([event_time(run_aff) for _ in range(reps)])
        jt.joint_from_affinities(idx, C)
        tp = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P = jt.joint_from_affinities(idx, C)
            torch.cuda.synchronize()
            tp.append(time.perf_counter() - t0)
        t_p = statistics.median(tp)
        nnz = int(P.col.numel())
        longest = int((P.rowptr[1:] - P.rowptr[:-1]).max().item())
        del idx, dist, C
        g = torch.Generator(device='cuda').manual_seed(1)
        Y = 30.0 * torch.randn(N, 2, device='cuda', generator=g)
        u = torch.zeros_like(Y)
        gain = torch.ones_like(Y)
        buf = jt._Gradient(N, Y.device, 0)
        kidx = torch.empty(N, 1, dtype=torch.int32, device='cuda')
        kdist = torch.empty(N, 1, dtype=torch.float32, device='cuda')
        cws = torch.empty(nv.metrics_workspace(N, N, 1), dtype=torch.uint8, device='cuda')

        def run_rep():
            nv.tsne_repulsion(Y, buf.R, buf.z, buf.Z, buf.ws_rep, 0)

        def run_cross():
            nv.cross_knn(Y, Y, 1, kidx, kdist, cws)

        def run_iter():                                    # (lr = 0 keeps the layout where it is: every round walks the same points)
            nv.tsne_repulsion(Y, buf.R, buf.z, buf.Z, buf.ws_rep, 0)
            nv.tsne_step(P.rowptr, P.col, P.val, Y, buf.R, buf.Z, 1.0, 0.8, 1e-30, u, gain, True, buf.ws_step)
        run_rep()
        run_cross()
        run_iter()
        torch.cuda.synchronize()
        tr, tc, ti = [], [], []
        for _ in range(reps):
            tr.append(event_time(run_rep))
            tc.append(event_time(run_cross))
            ti.append(event_time(run_iter))
        t_rep, t_cross, t_iter = statistics.median(tr), statistics.median(tc), statistics.median(ti)
        batch = a.batch if N < 500000 else max(1, a.batch // 10)
        tb = [event_time(lambda: [run_iter() for _ in range(batch)]) / batch for _ in range(min(reps, 3))]
        t_batch = statistics.median(tb)
        pairs = float(N) * N / t_rep
        r = {'pooled': N, 'L': L, 'K': K, 'reps': reps, 'repulsion_s': t_rep, 'repulsion_s_min_max': (min(tr), max(tr)),
             'cross_knn_k1_s': t_cross, 'cross_knn_k1_s_min_max': (min(tc), max(tc)), 'repulsion_over_cross': t_rep / t_cross,
             'iteration_s': t_iter, 'iteration_s_min_max': (min(ti), max(ti)), 'iteration_back_to_back_s': t_batch,
             'iterations_per_batch': batch, 'pairs_per_s': pairs, 'of_valu_issue_ceiling_per_instruction': pairs * VALU_PER_PAIR / ISSUE,
             'valu_per_pair': VALU_PER_PAIR, 'issue_slots_per_pair': SLOTS_PER_PAIR,
             'of_valu_issue_ceiling': pairs * SLOTS_PER_PAIR / ISSUE, 'affinities_s': t_aff, 'joint_p_wall_s': t_p, 'nnz': nnz, 'longest_row': longest, 'tries_max': int(tries.max().item()),
             'repulsion_workspace_bytes': nv.tsne_repulsion_workspace(N)}
        say(f"N={N}, L={L}, K={K}: repulsion {t_rep * 1e3:.3f} ms ({min(tr) * 1e3:.3f}-{max(tr) * 1e3:.3f}), {pairs / 1e12:.2f} T pairs/s, "
            f"{r['of_valu_issue_ceiling_per_instruction']:.3f} of the VALU issue ceiling at {VALU_PER_PAIR:.2f} instructions per pair "
            f"({r['of_valu_issue_ceiling']:.3f} if packed and v_rcp_f32 instructions are weighted as two slots, {SLOTS_PER_PAIR:.2f} per "
            f"pair: an assumption); cross_knn(Y, Y, 1) "
            f"{t_cross * 1e3:.3f} ms ({min(tc) * 1e3:.3f}-{max(tc) * 1e3:.3f}); repulsion / cross {r['repulsion_over_cross']:.3f}; whole "
            f"iteration {t_iter * 1e3:.3f} ms ({min(ti) * 1e3:.3f}-{max(ti) * 1e3:.3f}) alone, {t_batch * 1e3:.3f} ms each in {batch} back "
            f"to back; affinities {t_aff * 1e3:.3f} ms (at most "
            f"{r['tries_max']} tries); P build {t_p * 1e3:.1f} ms wall, nnz {nnz}, longest row {longest}; repulsion workspace "
            f"{r['repulsion_workspace_bytes'] / 2 ** 20:.1f} MiB")
        rows.append(r)
        del P, Y, u, gain, buf, kidx, kdist, cws
        torch.cuda.empty_cache()
    wall = None
    if a.wall_cells > 0:
        X = blobs(a.wall_cells, 32, 7)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = jt.tsne([X], perplexity=a.perplexity, n_iter=a.wall_iters)
        torch.cuda.synchronize()
        wall = {'cells': a.wall_cells, 'L': 32, 'n_iter': a.wall_iters, 'wall_s': time.perf_counter() - t0, 'kl': out['kl'],
                'kl_history': [float(v) for v in out['kl_history']]}
        say(f"tsne, {a.wall_cells} cells, L=32, {a.wall_iters} iterations, init 'pca': {wall['wall_s']:.2f} s wall, KL {out['kl']:.4f}")
        del X
    host = None
    if a.host_cells > 0:
        from sklearn.manifold import TSNE
        n = a.host_cells
        X = blobs(n, 32, 9).cpu().numpy()
        threads = int(os.environ.get('OMP_NUM_THREADS', '0')) or None
        t0 = time.perf_counter()
        sk = TSNE(method='barnes_hut', perplexity=a.perplexity, init='pca', n_jobs=threads).fit(X)
        t_sk = time.perf_counter() - t0
        t0 = time.perf_counter()
        dev = jt.tsne([X], perplexity=a.perplexity)
        torch.cuda.synchronize()
        t_dev = time.perf_counter() - t0
        host = {'cells': n, 'L': 32, 'threads': threads, 'sklearn_barnes_hut_s': t_sk, 'sklearn_kl': float(sk.kl_divergence_),
                'sklearn_n_iter': int(sk.n_iter_), 'device_s': t_dev, 'device_kl': dev['kl'], 'device_n_iter': dev['n_iter']}
        say(f"{n} cells, L=32: sklearn TSNE (barnes_hut, {threads} threads) {t_sk:.2f} s wall, {host['sklearn_n_iter']} iterations, KL "
            f"{host['sklearn_kl']:.4f}; tsne {t_dev:.2f} s wall, {dev['n_iter']} iterations, KL {dev['kl']:.4f}")
    say(json.dumps({'bench_tsne': rows, 'tsne_wall': wall, 'sklearn': host}))
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

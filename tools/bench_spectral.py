"""Spectral embedding on the device: the step of the filter, the Gram matrix, the rotation and the whole call, on resident inputs.

    python tools/bench_spectral.py [--cases 200000x32,1000000x32] [--wall-cells 200000] [--eigsh-limit 300] [--log PATH]

Without --child the tool only starts one fresh process per case (two more for the whole-call timing, on one connected graph and
on blobs that fall into separate components, and one, on the CPU alone, for `scipy.sparse.linalg.eigsh` on the connected matrix),
each under its own time limit, and stops at the first GPU step that fails; it does not touch the GPU itself.  A child (--child NxL) measures with HIP events around the C-ABI calls, median of --reps rounds after a
warm-up round, for B = 16 and 32:

    alternating in the same process: one `jamie_graph_cheb_step` (with `prev`), `jamie_tsne_step`'s attraction pass over the same
        CSR arrays (the same rows walked by one wave each), and a device copy of the bytes the step must touch at least once: the
        CSR arrays (8 (N + 1) + 8 nnz), the scale (8 N) and three blocks (in, prev, out: 24 N B); bytes/s and the share of the copy's
    one `jamie_block_gram` and one `jamie_block_rotate` on the same blocks

No time is fixed in advance; what a run did not measure is written as such.  Prints one line per case, a JSON line at the end, and
appends both to --log."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def child_case(N, L, a, say):
    import torch
    from bench_umap import blobs, event_time
    from jamie_amd import _native as nv
    from jamie_amd import spectral as js
    from jamie_amd import tsne as jt
    nn = a.n_neighbors
    reps = a.reps if N < 500000 else 3
    G = js.build_graph(blobs(N, L, N + L), nn)
    nnz = int(G.col.numel())
    longest = int((G.rowptr[1:] - G.rowptr[:-1]).max().item())
    scale, _ = js.normalised_operator(G, False)
    buf = jt._Gradient(N, G.col.device, 0)
    buf.R.zero_()
    buf.Z.fill_(1.0)
    Yt = torch.rand(N, 2, device='cuda') * 10.0
    grad = torch.empty(N, 2, dtype=torch.float32, device='cuda')
    out = {'pooled': N, 'L': L, 'n_neighbors': nn, 'reps': reps, 'nnz': nnz, 'longest_row': longest}

    def run_attract():
        nv.tsne_step(G.rowptr, G.col, G.val, Yt, buf.R, buf.Z, 1.0, 0.0, 1.0, None, None, False, buf.ws_step, grad=grad)
    for B in (16, 32):
        g = torch.Generator(device='cuda').manual_seed(B)
        X, P, O = (torch.randn(N, B, dtype=torch.float64, device='cuda', generator=g) for _ in range(3))
        M = torch.randn(B, B, dtype=torch.float64, device='cuda', generator=g)
        ws = torch.empty(nv.block_gram_workspace(N, B) // 8, dtype=torch.float64, device='cuda')
        H = torch.empty(B, B, dtype=torch.float64, device='cuda')
        touched = 8 * (N + 1) + 8 * nnz + 8 * N + 24 * N * B
        src = torch.empty(touched // 2, dtype=torch.uint8, device='cuda')
        dst = torch.empty_like(src)

        def run_step():
            js.cheb_step(G, scale, X, P, O, 1.1, -0.2, 0.3)

        def run_copy():
            dst.copy_(src)

        def run_gram():
            nv.block_gram(X, P, ws, H)

        def run_rotate():
            nv.block_rotate(X, M, None, None, O)
        for warm in (run_step, run_attract, run_copy, run_gram, run_rotate):
            warm()
        torch.cuda.synchronize()
        ts, ta, tc, tg, tr = [], [], [], [], []
        for _ in range(reps):
            ts.append(event_time(run_step))
            ta.append(event_time(run_attract))
            tc.append(event_time(run_copy))
            tg.append(event_time(run_gram))
            tr.append(event_time(run_rotate))
        t_step, t_att, t_copy, t_gram, t_rot = (statistics.median(t) for t in (ts, ta, tc, tg, tr))
        gathered = 8 * (N + 1) + 8 * nnz + 8 * N + 8 * nnz + 8 * B * nnz + 24 * N * B      # with every gathered line and scale counted
        out[f'B{B}'] = {'cheb_step_s': t_step, 'cheb_step_s_min_max': (min(ts), max(ts)), 'bytes_touched': touched,
                        'bytes_per_s': touched / t_step, 'bytes_gathered': gathered, 'gathered_bytes_per_s': gathered / t_step,
                        'copy_same_bytes_s': t_copy, 'copy_bytes_per_s': touched / t_copy, 'share_of_copy': t_copy / t_step,
                        'tsne_attraction_s': t_att, 'step_over_attraction': t_step / t_att, 'gram_s': t_gram, 'rotate_s': t_rot}
        say(f"N={N}, L={L}, n_neighbors={nn}, B={B}: nnz {nnz}, longest row {longest}; cheb_step {t_step * 1e3:.3f} ms "
            f"({min(ts) * 1e3:.3f}-{max(ts) * 1e3:.3f}): {touched / t_step / 1e12:.3f} TB/s of the {touched / 1e6:.1f} MB it must touch "
            f"({gathered / t_step / 1e12:.3f} TB/s counting every gathered row, {gathered / 1e6:.1f} MB); a device copy of the touched "
            f"bytes {t_copy * 1e3:.3f} ms ({touched / t_copy / 1e12:.2f} TB/s): the step runs at {t_copy / t_step:.2f} of the copy's rate; "
            f"t-SNE attraction pass over the same rows {t_att * 1e3:.3f} ms (step / attraction {t_step / t_att:.2f}); gram "
            f"{t_gram * 1e3:.3f} ms, rotate {t_rot * 1e3:.3f} ms")
        del X, P, O, src, dst, ws
    return out


def overlapping(N, L, seed, n_blobs=40):
    """Blobs whose centres are as far apart as two cells of one blob: one connected graph (bench_umap's blobs, twice as far
    apart, fall into separate components at these sizes)."""
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    lab = torch.randint(0, n_blobs, (N,), device='cuda', generator=g)
    return torch.randn(n_blobs, L, device='cuda', generator=g)[lab] + torch.randn(N, L, device='cuda', generator=g)


def child_wall(N, a, say, apart=False):
    import numpy as np
    import torch
    from bench_umap import blobs
    from jamie_amd import spectral as js
    X = blobs(N, 32, 7) if apart else overlapping(N, 32, 7)
    say(f"cells: {'40 blobs apart (separate components)' if apart else '40 overlapping blobs (one graph)'}")
    js.spectral([X[:4096]])                                  # (the library is loaded, the allocator is warm)
    res = {'wall_cells': N, 'L': 32, 'n_neighbors': a.n_neighbors}
    for kind, nc in (('laplacian', 2), ('diffmap', 10)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = js.spectral([X], n_components=nc, n_neighbors=a.n_neighbors, kind=kind,
                          return_graph=bool(a.save_graph) and nc == 2 and not apart)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        say(f"spectral, {N} cells, L=32, n_neighbors={a.n_neighbors}, kind={kind}, n_components={nc}: {wall:.2f} s wall, "
            f"{out['n_edges']} edges, converged {out['converged']}, {out['iterations']} outer iterations, {out['applies']} applies, "
            f"degrees {out['degrees']}, eigenvalues {out['eigenvalues'][0]:.9f} .. {out['eigenvalues'][-1]:.9f}, largest residual "
            f"{out['residuals'].max():.2e}")
        res[kind] = {'n_components': nc, 'wall_s': wall, 'converged': out['converged'], 'iterations': out['iterations'],
                     'applies': out['applies'], 'degrees': out['degrees'], 'eigenvalues': [float(v) for v in out['eigenvalues']],
                     'residual_max': float(out['residuals'].max())}
        if out['graph'] is not None:
            g = out['graph']
            np.savez(a.save_graph, indptr=g.indptr, indices=g.indices, data=g.data, n=N)
    return res


def child_eigsh(a, say):
    """scipy's ARPACK on the same matrix, on the CPU alone (this process never opens the GPU)."""
    import numpy as np
    from scipy.sparse import csr_matrix, diags
    from scipy.sparse.linalg import eigsh
    z = np.load(a.save_graph)
    N = int(z['n'])
    A = csr_matrix((z['data'].astype(np.float64), z['indices'], z['indptr']), shape=(N, N))
    s = 1.0 / np.sqrt(np.asarray(A.sum(axis=1)).ravel())
    S = diags(s) @ A @ diags(s)
    t0 = time.perf_counter()
    w, _ = eigsh(S, k=3, which='LA', tol=1e-8, v0=np.random.default_rng(0).standard_normal(N))
    wall = time.perf_counter() - t0
    say(f'scipy.sparse.linalg.eigsh (k = 3, which = LA, tol = 1e-8) on the same {N}-cell matrix, host CPU: {wall:.2f} s wall, eigenvalues '
        f'{sorted(w.tolist(), reverse=True)}')
    return {'cells': N, 'wall_s': wall, 'eigenvalues': sorted(w.tolist(), reverse=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='200000x32,1000000x32', help='pooled cells x L')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--n-neighbors', type=int, default=15)
    ap.add_argument('--wall-cells', type=int, default=200000, help='cells of the whole-call timing (0: skip)')
    ap.add_argument('--limit', type=int, default=240, help='seconds a GPU child may take')
    ap.add_argument('--eigsh-limit', type=int, default=300, help='seconds the eigsh child may take (0: skip)')
    ap.add_argument('--child', default=None, help='(internal) NxL, wallN, apartN or eigsh')
    ap.add_argument('--save-graph', default='', help='(internal) the .npz the whole-call child leaves for the eigsh child')
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'bench_spectral.log'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    if a.child is None:
        open(a.log, 'w').close()
        with tempfile.TemporaryDirectory() as tmp:
            graph = os.path.join(tmp, 'graph.npz')
            steps = a.cases.split(',') + ([f'wall{a.wall_cells}', f'apart{a.wall_cells}'] if a.wall_cells > 0 else [])
            base = [sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), '--n-neighbors', str(a.n_neighbors), '--log', a.log,
                    '--save-graph', graph if a.eigsh_limit > 0 else '']
            for step in steps:                              # one fresh process per step, each under its own limit; stop at a failure
                rc = subprocess.run(base + ['--child', step], timeout=a.limit).returncode
                if rc != 0:
                    sys.exit(f'bench_spectral: step {step} ended with status {rc}; nothing further was started')
            if a.eigsh_limit > 0 and os.path.exists(graph):
                try:
                    subprocess.run(base + ['--child', 'eigsh'], timeout=a.eigsh_limit)
                except subprocess.TimeoutExpired:
                    with open(a.log, 'a') as f:
                        f.write(f'scipy.sparse.linalg.eigsh: not finished within {a.eigsh_limit} s on the host CPU; NOT MEASURED\n')
                    print(f'eigsh: not finished within {a.eigsh_limit} s; not measured', flush=True)
            else:
                with open(a.log, 'a') as f:
                    f.write('scipy.sparse.linalg.eigsh: NOT MEASURED (skipped)\n')
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if a.child == 'eigsh':
        out = {'eigsh': child_eigsh(a, say)}
    else:
        import torch
        from jamie_amd import _native as nv
        nv.require_gpu()
        prop = torch.cuda.get_device_properties(0)
        say(f'device: {prop.name}, {prop.multi_processor_count} CUs')
        if a.child.startswith('wall'):
            out = {'spectral_wall': child_wall(int(a.child[4:]), a, say)}
        elif a.child.startswith('apart'):
            out = {'spectral_wall_apart': child_wall(int(a.child[5:]), a, say, apart=True)}
        else:
            N, L = (int(v) for v in a.child.split('x'))
            out = {'bench_spectral': child_case(N, L, a, say)}
    say(json.dumps(out))
    with open(a.log, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

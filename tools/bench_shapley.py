"""Shapley attributions on the device against the loop a user would write, at the BASELINE config 2 widths.

    python tools/bench_shapley.py [--dims 2000,1000] [--latent 32] [--cells 8192] [--orders 4] [--loop-sample 48] [--reps 3]
                                  [--max-workspace 1073741824] [--max-accumulator 1073741824] [--cases i,ii]

A model with random weights and randomised BatchNorm statistics, `--cells` standardised random cells of modality 0 resident on the
device, attributions towards modality 1 in two cases:
  (i)   every input feature a player (2000), 8 target columns;
  (ii)  256 players spread over the range, all target columns (1000),
both over `--orders` orders (half drawn, half their reverses).  Wall time around calls that end in a device-to-host copy (so the
device work is inside), one warm-up call per case with the timed call's chunk and segment sizes, then --reps rounds that run the
two routes one after the other (interleaved), the median of each:
  device route   `jamie_amd.shapley.shapley_values`: seconds and rows (cell prefixes pushed through the network) per second;
  loop route     per (order, prefix): clone the resident cells, set the removed players to the background on the device,
                 `model.impute`, the target columns to float64 -- on `--loop-sample` (order, prefix) pairs spread over the walks,
                 timed, and EXTRAPOLATED to all orders x (players + 1) prefixes by that ratio (labelled as such: it is no measurement
                 of the full loop);
an agreement check of the two routes on 512 cells, 8 players and one order; and the walk kernel alone (device events, median of 5)
at case (i)'s chunk and segment size: its achieved store bandwidth beside a device copy of the same bytes.  Prints one line per
figure and a JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jamie_amd import _native as nv  # noqa: E402
from jamie_amd import shapley as sh  # noqa: E402
from jamie_amd.model import BN_EPS, LRELU_SLOPE, edModelVar  # noqa: E402


def randomise_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    sd = model.state_dict()
    for k in list(sd):
        if k.endswith('.running_mean'):
            pre, n = k[:-len('.running_mean')], sd[k].numel()
            sd[pre + '.running_mean'] = 0.3 * torch.randn(n, generator=g)
            sd[pre + '.running_var'] = torch.empty(n).uniform_(0.5, 2.0, generator=g)
            sd[pre + '.weight'] = torch.empty(n).uniform_(0.5, 1.5, generator=g)
            sd[pre + '.bias'] = 0.2 * torch.randn(n, generator=g)
    model.load_state_dict(sd)


def wall_once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def loop_pairs(model, X, bg, feat, orders, pairs, tcol, i, t):
    """The loop route's work for the (order, prefix length) pairs: the masked input of each built on the device, `model.impute`, the
    target columns in float64, brought to the host at the end."""
    cols = torch.as_tensor(np.asarray(tcol, dtype=np.int64), device=X.device)
    keep = []
    for q, m in pairs:
        Xm = X.clone()
        gone = torch.as_tensor(feat[orders[q, :m]].astype(np.int64), device=X.device)
        Xm[:, gone] = bg[gone]
        keep.append(model.impute(Xm, [i, t])[:, cols].double().sum(0))
    return torch.stack(keep).cpu().numpy()


def loop_values(model, X, bg, feat, orders, tcol, i, t):
    """values [N, F, T] by the loop route (every prefix of every order), float64 on the device."""
    cols = torch.as_tensor(np.asarray(tcol, dtype=np.int64), device=X.device)
    out = torch.zeros(X.shape[0], len(feat), len(tcol), dtype=torch.float64, device=X.device)
    for o in orders:
        Xm = X.clone()
        prev = model.impute(Xm, [i, t])[:, cols].double()
        for k in o:
            Xm[:, int(feat[k])] = bg[int(feat[k])]
            cur = model.impute(Xm, [i, t])[:, cols].double()
            out[:, int(k)] += prev - cur
            prev = cur
    return (out / len(orders)).cpu().numpy()


def walk_kernel_alone(model, X, bg, n, g, i):
    """Median device time of jamie_shapley_walk_rows on n cells x g steps, and of a device copy of the bytes it stores."""
    W0, b0 = model.p[f'm{i}.enc0.W'], model.p[f'm{i}.enc0.b']
    bn0 = tuple(model.bn[f'm{i}.bn0.{k}'] for k in ('mean', 'var')) + tuple(model.p[f'm{i}.bn0.{k}'] for k in ('g', 'b'))
    h, d = W0.shape[0], X.shape[1]
    x = X[:n]
    H = model._linear(x, W0, b0)
    state = H.clone()
    out = torch.empty((g + 1) * n, h, device=X.device)
    src = torch.empty_like(out)
    ws = torch.empty(nv.shapley_walk_workspace(g, h), dtype=torch.uint8, device=X.device)
    feat = np.linspace(0, d - 1, g).astype(np.int32)
    feat_dev = torch.from_numpy(feat).to(X.device)

    def walk():
        nv.shapley_walk_rows(state, x, bg, W0, feat, bn0, out, ws, h=h, d=d, eps=BN_EPS, slope=LRELU_SLOPE, feat_dev=feat_dev)

    def copy():
        out.copy_(src)
    res = {}
    for name, fn in (('walk', walk), ('copy', copy)):
        fn()
        ts = []
        for _ in range(5):
            state.copy_(H)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        res[name] = statistics.median(ts)
    return res, out.numel() * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dims', default='2000,1000')
    ap.add_argument('--latent', type=int, default=32)
    ap.add_argument('--cells', type=int, default=8192)
    ap.add_argument('--orders', type=int, default=4)
    ap.add_argument('--loop-sample', type=int, default=48)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--max-workspace', type=int, default=1 << 30)
    ap.add_argument('--max-accumulator', type=int, default=1 << 30)
    ap.add_argument('--cases', default='i,ii')
    a = ap.parse_args()
    nv.require_gpu()
    dims = [int(v) for v in a.dims.split(',')]
    i, t = 0, 1
    prop = torch.cuda.get_device_properties(0)
    torch.manual_seed(0)
    model = edModelVar(dims, a.latent).eval()
    randomise_bn(model, 1)
    d_i, d_t = dims[i], dims[t]
    gen = torch.Generator(device='cuda').manual_seed(2)
    X = torch.randn(a.cells, d_i, device='cuda', generator=gen)
    bg = torch.zeros(d_i, device='cuda')
    caps = dict(max_workspace=a.max_workspace, max_accumulator=a.max_accumulator)
    P = max(1, a.orders)
    print(f'device: {prop.name}, {prop.multi_processor_count} CUs; dims {dims}, latent {a.latent}, {a.cells} cells of modality {i} towards '
          f'modality {t}, {P} orders; median of {a.reps} interleaved rounds after a warm-up', flush=True)
    cases = {'i': (np.arange(d_i), np.linspace(0, d_t - 1, min(8, d_t)).astype(np.int64)),
             'ii': (np.unique(np.linspace(0, d_i - 1, min(256, d_i)).astype(np.int64)), np.arange(d_t))}
    report = {'dims': dims, 'latent': a.latent, 'cells': a.cells, 'orders': P}
    for name in a.cases.split(','):
        feat, tcol = cases[name]
        F, T = len(feat), len(tcol)
        orders = sh.draw_orders(F, (P + 1) // 2, antithetic=P > 1, seed=0)[:P]
        p = sh.plan(a.cells, d_i, d_t, F, T, **caps)
        rows = P * sum(nc * (gc + 1) for _, nc in p['chunks'] for _, gc in p['segments'])
        print(f'case ({name}): {F} players, {T} targets; plan: {len(p["chunks"])} chunk(s) of {p["n"]} cells x {len(p["segments"])} '
              f'segment(s) of {p["g"]} steps, widest activation {p["workspace"]} bytes, accumulator {p["accumulator"]} bytes; {rows} rows',
              flush=True)
        S = max(1, min(a.loop_sample, P * (F + 1)))
        pairs = [(int(k) // (F + 1), int(k) % (F + 1)) for k in np.unique(np.linspace(0, P * (F + 1) - 1, S).astype(np.int64))]
        # warm-up: one order of the timed call (the same chunk and segment sizes), and two pairs of the loop
        sh.shapley_values(model, X, i, t, background=bg, features=feat, targets=tcol, orders=orders[:1], **caps)
        loop_pairs(model, X, bg, feat, orders, pairs[:2], tcol, i, t)
        td, tl, out = [], [], {}
        for _ in range(a.reps):
            td.append(wall_once(lambda: out.update(r=sh.shapley_values(model, X, i, t, background=bg, features=feat, targets=tcol,
                                                                       orders=orders, **caps))))
            tl.append(wall_once(lambda: loop_pairs(model, X, bg, feat, orders, pairs, tcol, i, t)))
        d_med, l_med = statistics.median(td), statistics.median(tl)
        scale = P * (F + 1) / len(pairs)
        print(f'case ({name}) device route: {d_med:.3f} s ({min(td):.3f}-{max(td):.3f}) for {rows} rows = {rows / d_med / 1e6:.2f} M rows/s',
              flush=True)
        print(f'case ({name}) loop route (device-resident inputs, model.impute per prefix): {l_med:.3f} s ({min(tl):.3f}-{max(tl):.3f}) for '
              f'{len(pairs)} sampled (order, prefix) pairs; EXTRAPOLATED to {P} x {F + 1} prefixes: {l_med * scale:.3f} s = '
              f'{P * (F + 1) * a.cells / (l_med * scale) / 1e6:.2f} M rows/s', flush=True)
        print(f'case ({name}) device route against the extrapolated loop: {l_med * scale / d_med:.2f}x; mean importance '
              f'{float(out["r"]["importance"].mean()):.6e}', flush=True)
        report[name] = {'players': F, 'targets': T, 'plan': {k: p[k] for k in ('n', 'g', 'rows', 'workspace', 'accumulator')},
                        'rows': rows, 'device_s': d_med, 'device_s_min_max': (min(td), max(td)), 'device_rows_per_s': rows / d_med,
                        'loop_sample': len(pairs), 'loop_sample_s': l_med, 'loop_sample_s_min_max': (min(tl), max(tl)),
                        'loop_extrapolated_s': l_med * scale, 'speedup_vs_extrapolated_loop': l_med * scale / d_med}
    # agreement of the two routes where the full loop is cheap
    feat, tcol = np.linspace(0, d_i - 1, 8).astype(np.int64), np.linspace(0, d_t - 1, 8).astype(np.int64)
    orders = sh.draw_orders(8, 1, antithetic=False, seed=1)
    n_chk = min(512, a.cells)
    va = sh.shapley_values(model, X[:n_chk], i, t, background=bg, features=feat, targets=tcol, orders=orders, return_values=True)['values']
    vb = loop_values(model, X[:n_chk], bg, feat, orders, tcol, i, t)
    diff = float(np.abs(va - vb).max() / np.abs(vb).max())
    ymax = float(model.impute(X[:n_chk], [i, t]).abs().max())
    print(f'agreement on {n_chk} cells, 8 players, 8 targets, 1 order: largest difference of values over the largest value {diff:.2e} '
          f'(largest |value| {float(np.abs(vb).max()):.2e}: the difference is {float(np.abs(va - vb).max()) / ymax:.2e} of the largest '
          f'imputed value {ymax:.2f}, whose fp32 products both routes difference)', flush=True)
    p = sh.plan(a.cells, d_i, d_t, d_i, min(8, d_t), **caps)
    res, stored = walk_kernel_alone(model, X, bg, p['n'], p['g'], i)
    print(f'walk kernel alone, {p["n"]} cells x {p["g"]} steps, h = {2 * d_i}: {res["walk"] * 1e3:.3f} ms for {stored} bytes stored = '
          f'{stored / res["walk"] / 1e12:.2f} TB/s of stores (it also reads the state and, from cache, W0^T); a device copy of the same '
          f'bytes: {res["copy"] * 1e3:.3f} ms = {stored / res["copy"] / 1e12:.2f} TB/s written (and as much read)')
    report.update(agreement=diff, walk_s=res['walk'], walk_bytes_stored=stored, walk_store_bytes_per_s=stored / res['walk'],
                  copy_s=res['copy'], copy_bytes_per_s=stored / res['copy'])
    print(json.dumps({'bench_shapley': report}))


if __name__ == '__main__':
    main()

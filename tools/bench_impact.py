"""Feature impact on the device against the loop a user would write, at the BASELINE config 2 widths.

    python tools/bench_impact.py [--dims 2000,1000] [--latent 32] [--cells 8192] [--features 0 (all)] [--loop-sample 48]
                                 [--reps 3] [--max-workspace 1073741824]

A model with random weights and randomised BatchNorm statistics, `--cells` standardised random cells of modality 0 resident on the
device, every input feature occluded towards modality 1.  Wall time around calls that end in a device-to-host copy (so the device
work is inside), one warm-up call on a few features, the median of --reps calls:
  device route   `jamie_amd.impact.feature_impact` on all features: seconds, occluded rows (features x cells) per second, and the
                 FLOP/s of the products it needs (everything after the first layer per occluded row, the whole network once per cell);
  loop route     per feature: clone the resident cells, replace the column on the device, `model.impute`, the squared differences
                 averaged on the device in float64 -- on `--loop-sample` features spread over the range, timed, and EXTRAPOLATED to all
                 features by features / sample (labelled as such: it is no measurement of the full loop);
and the largest difference between the two routes on the sampled features relative to the largest value.  Prints one line per
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
from jamie_amd import impact as fi  # noqa: E402
from jamie_amd.model import edModelVar  # noqa: E402


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


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def loop_route(model, X, bg, feats, i, t):
    Y = model.impute(X, [i, t]).double()
    rows = []
    for f in feats:
        Xm = X.clone()
        Xm[:, f] = bg[f]
        rows.append(((model.impute(Xm, [i, t]).double() - Y) ** 2).mean(0))
    return torch.stack(rows).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dims', default='2000,1000')
    ap.add_argument('--latent', type=int, default=32)
    ap.add_argument('--cells', type=int, default=8192)
    ap.add_argument('--features', type=int, default=0, help='occlude the first K features (0: all)')
    ap.add_argument('--loop-sample', type=int, default=48)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--max-workspace', type=int, default=1 << 30)
    a = ap.parse_args()
    nv.require_gpu()
    dims = [int(v) for v in a.dims.split(',')]
    i, t = 0, 1
    prop = torch.cuda.get_device_properties(0)
    torch.manual_seed(0)
    model = edModelVar(dims, a.latent).eval()
    randomise_bn(model, 1)
    d_i, d_t, L = dims[i], dims[t], a.latent
    F = d_i if a.features <= 0 else min(a.features, d_i)
    feats = np.arange(F)
    gen = torch.Generator(device='cuda').manual_seed(2)
    X = torch.randn(a.cells, d_i, device='cuda', generator=gen)
    bg = torch.zeros(d_i, device='cuda')
    p = fi.plan(a.cells, d_i, d_t, F, a.max_workspace)
    print(f'device: {prop.name}, {prop.multi_processor_count} CUs; dims {dims}, latent {L}, {a.cells} cells, {F} features of modality {i} '
          f'towards modality {t}; plan: {len(p["chunks"])} chunk(s) of {p["n"]} cells x {len(p["groups"])} group(s) of {p["g"]} features, '
          f'widest activation {p["workspace"]} bytes; median of {a.reps} calls after a warm-up')
    rest = 2 * (2 * d_i * d_i + d_i * L + L * d_t + 2 * d_t * d_t + 2 * d_t * d_t)      # FLOPs per row after the first layer
    first = 2 * 2 * d_i * d_i
    flops = F * a.cells * rest + a.cells * (2 * first + rest)

    fi.feature_impact(model, X, i, t, background=bg, features=feats[:min(F, 2 * fi.GROUP)], max_workspace=a.max_workspace)      # warm-up
    out = {}

    def device_route():
        out['r'] = fi.feature_impact(model, X, i, t, background=bg, features=feats, max_workspace=a.max_workspace)
    td = wall(device_route, a.reps)
    rows = F * a.cells
    print(f'device route: {td[0]:.3f} s ({td[1]:.3f}-{td[2]:.3f}) for {rows} occluded rows = {rows / td[0] / 1e6:.2f} M rows/s, '
          f'{flops / td[0] / 1e12:.1f} TFLOP/s of the products it needs', flush=True)

    S = max(1, min(a.loop_sample, F))
    sample = np.unique(np.linspace(0, F - 1, S).astype(np.int64))
    loop_route(model, X, bg, sample[:2], i, t)                                           # warm-up
    lo = {}

    def loop():
        lo['r'] = loop_route(model, X, bg, sample, i, t)
    tl = wall(loop, a.reps)
    scale = F / len(sample)
    print(f'loop route (device-resident inputs, model.impute per feature): {tl[0]:.3f} s ({tl[1]:.3f}-{tl[2]:.3f}) for {len(sample)} '
          f'sampled features; EXTRAPOLATED to {F} features: {tl[0] * scale:.3f} s = {rows / (tl[0] * scale) / 1e6:.2f} M rows/s', flush=True)
    diff = float(np.abs(out['r']['per_target'][sample] - lo['r']).max() / lo['r'].max())
    ratio = tl[0] * scale / td[0]
    print(f'device route against the extrapolated loop: {ratio:.2f}x; largest difference of per_target on the sampled features over '
          f'the largest value: {diff:.2e}')
    print(json.dumps({'bench_impact': {'dims': dims, 'latent': L, 'cells': a.cells, 'features': F, 'plan': {k: p[k] for k in ('n', 'g', 'rows', 'workspace')},
                                       'device_s': td[0], 'device_s_min_max': td[1:], 'device_rows_per_s': rows / td[0],
                                       'device_flops_per_s': flops / td[0], 'loop_sample': len(sample), 'loop_sample_s': tl[0],
                                       'loop_sample_s_min_max': tl[1:], 'loop_extrapolated_s': tl[0] * scale,
                                       'loop_extrapolated_rows_per_s': rows / (tl[0] * scale), 'speedup_vs_extrapolated_loop': ratio,
                                       'max_relative_difference': diff, 'mean_impact': float(out['r']['impact'].mean())}}))


if __name__ == '__main__':
    main()

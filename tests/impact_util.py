"""Float64 numpy restatement of the eval-mode network from `state_dict()` and of the feature-impact definition
(jamie_amd/impact.py), shared by test_host_impact.py and test_hip_impact.py.  Nothing here touches a GPU except `randomise_bn`,
`loop_route` and the model fixtures' callers."""
import numpy as np

from oracle.jamie_oracle import BN_EPS, LRELU_SLOPE


def weights64(sd):
    """state_dict (reference names, tensors or arrays) -> {name: float64 numpy}."""
    return {k: np.asarray(v.detach().cpu() if hasattr(v, 'detach') else v, dtype=np.float64) for k, v in sd.items()}


def bn_act(v, W, name):
    """eval BatchNorm1d + LeakyReLU of the block whose BatchNorm is `name`."""
    y = (v - W[name + '.running_mean']) / np.sqrt(W[name + '.running_var'] + BN_EPS) * W[name + '.weight'] + W[name + '.bias']
    return np.where(y > 0, y, LRELU_SLOPE * y)


def lin(v, W, name):
    return v @ W[name + '.weight'].T + W[name + '.bias']


def pre0(W, i, X):
    """W0 x + b of encoder i: the first layer before BatchNorm."""
    return lin(np.asarray(X, dtype=np.float64), W, f'encoders.{i}.0')


def impute_from_pre(W, H, i, t):
    """decoders[t](fc_mus[i](rest of encoders[i])) from the first layer's pre-activation H."""
    a = bn_act(H, W, f'encoders.{i}.1')
    a = bn_act(lin(a, W, f'encoders.{i}.4'), W, f'encoders.{i}.5')
    z = lin(a, W, f'fc_mus.{i}')
    a = bn_act(lin(z, W, f'decoders.{t}.0'), W, f'decoders.{t}.1')
    a = bn_act(lin(a, W, f'decoders.{t}.4'), W, f'decoders.{t}.5')
    return lin(a, W, f'decoders.{t}.8')


def impute64(W, X, i, t):
    return impute_from_pre(W, pre0(W, i, X), i, t)


def occluded_by_replacement(W, X, i, t, f, bg):
    Xm = np.array(X, dtype=np.float64)
    Xm[:, f] = bg[f]
    return impute64(W, Xm, i, t)


def occluded_by_rank_one(W, X, i, t, f, bg, H=None):
    X = np.asarray(X, dtype=np.float64)
    H = pre0(W, i, X) if H is None else H
    return impute_from_pre(W, H + (bg[f] - X[:, f])[:, None] * W[f'encoders.{i}.0.weight'][:, f][None, :], i, t)


def reference(W, X, i, t, bg, feat, measured=None):
    """(per_target [F, d_t], baseline [d_t] or None) by the definition: the column is replaced, everything in float64."""
    X = np.asarray(X, dtype=np.float64)
    bg = np.asarray(bg, dtype=np.float64)
    Y = impute64(W, X, i, t)
    R = Y if measured is None else np.asarray(measured, dtype=np.float64)
    per = np.stack([((occluded_by_replacement(W, X, i, t, int(f), bg) - R) ** 2).mean(0) for f in feat])
    return per, (None if measured is None else ((Y - R) ** 2).mean(0))


def err(per_target, ref):
    """The issue's error measure: max |per_target - ref| / max ref."""
    return float(np.abs(np.asarray(per_target) - ref).max() / ref.max())


def random_bn(rng, n, var_lo=0.5, var_hi=2.0):
    """(running mean, running var, gamma, beta) float32 [n]: variances log-uniform in [var_lo, var_hi]."""
    return ((0.3 * rng.standard_normal(n)).astype(np.float32),
            np.exp(rng.uniform(np.log(var_lo), np.log(var_hi), n)).astype(np.float32),
            rng.uniform(0.5, 1.5, n).astype(np.float32), (0.2 * rng.standard_normal(n)).astype(np.float32))


def randomise_bn_state(sd, seed):
    """The state_dict `sd` with every BatchNorm's running statistics and affine pair drawn at random (in place; returns sd)."""
    import torch
    rng = np.random.default_rng(seed)
    for k in list(sd):
        if k.endswith('.running_mean'):
            pre = k[:-len('.running_mean')]
            m, v, g, b = random_bn(rng, sd[k].numel())
            for name, val in ((pre + '.running_mean', m), (pre + '.running_var', v), (pre + '.weight', g), (pre + '.bias', b)):
                sd[name] = torch.from_numpy(val).to(sd[name].device)
    return sd


def loop_route(model, X, i, t, bg, feat, measured=None):
    """Route (b): per feature, replace the column on the device and call `model.impute`; the squared differences are averaged in
    float64, so what separates it from the float64 restatement is the network's fp32 arithmetic alone."""
    import torch
    Xd = torch.as_tensor(np.asarray(X, dtype=np.float32)).to(model.device)
    Y = model.impute(Xd, [i, t]).double()
    R = Y if measured is None else torch.as_tensor(np.asarray(measured, dtype=np.float32)).to(model.device).double()
    rows = []
    for f in feat:
        Xm = Xd.clone()
        Xm[:, int(f)] = float(np.float32(bg[int(f)]))
        rows.append(((model.impute(Xm, [i, t]).double() - R) ** 2).mean(0))
    return torch.stack(rows).cpu().numpy(), (None if measured is None else ((Y - R) ** 2).mean(0).cpu().numpy())

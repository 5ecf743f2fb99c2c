"""Float64 references for the Shapley attributions (jamie_amd/shapley.py), shared by test_host_shapley.py and test_hip_shapley.py:
the exact Shapley value by enumeration of all 2^F coalitions, the float64 walk for given orders, and the loop route that builds
every masked input on the device and calls `model.impute`.  Value functions are callables `v(Xm) -> [N, T]` on masked inputs; the
network's is `network_value` on `impact_util`'s float64 restatement.  Nothing here touches a GPU except `loop_route`."""
import itertools
import math

import numpy as np

import impact_util as fu


def network_value(W, i, t, tcol=None):
    """v(Xm) = the float64 imputation i -> t of the masked cells Xm, columns `tcol` (None: all)."""
    def v(Xm):
        Y = fu.impute_from_pre(W, fu.pre0(W, i, Xm), i, t)
        return Y if tcol is None else Y[:, list(tcol)]
    return v


def masked(X, bg, feat, present):
    """The cells with every player NOT in the coalition `present` (a boolean [F]) set to its background."""
    Xm = np.array(X, dtype=np.float64)
    for k, f in enumerate(feat):
        if not present[k]:
            Xm[:, int(f)] = bg[int(f)]
    return Xm


def exact_shapley(v, X, bg, feat):
    """values [N, F, T] by the definition: phi_k = sum over S not containing k of |S|! (F - |S| - 1)! / F! (v(S + k) - v(S)),
    every coalition evaluated once, float64."""
    F = len(feat)
    val = {}
    for bits in itertools.product((False, True), repeat=F):
        val[bits] = v(masked(X, bg, feat, bits))
    out = np.zeros((np.asarray(X).shape[0], F, val[(False,) * F].shape[1]))
    for bits, vs in val.items():
        size = sum(bits)
        for k in range(F):
            if not bits[k]:
                wgt = math.factorial(size) * math.factorial(F - size - 1) / math.factorial(F)
                out[:, k] += wgt * (val[bits[:k] + (True,) + bits[k + 1:]] - vs)
    return out


def walk64(v, X, bg, feat, orders):
    """values [N, F, T]: the mean over `orders` [P, F] of the removal walk's contributions, float64."""
    F = len(feat)
    out = None
    for o in np.asarray(orders):
        present = [True] * F
        prev = v(masked(X, bg, feat, present))
        if out is None:
            out = np.zeros((prev.shape[0], F, prev.shape[1]))
        for k in o:
            present[int(k)] = False
            cur = v(masked(X, bg, feat, present))
            out[:, int(k)] += prev - cur
            prev = cur
    return out / len(orders)


def all_orders(F):
    return np.array(list(itertools.permutations(range(F))), dtype=np.int32)


def loop_route(model, X, i, t, bg, feat, orders, tcol=None):
    """Route (b): for the same orders, every masked input is built on the device and goes through `model.impute`; differences and
    means are taken in float64, so what separates it from the float64 walk is the network's fp32 arithmetic alone."""
    import torch
    Xd = torch.as_tensor(np.asarray(X, dtype=np.float32)).to(model.device)
    bgd = torch.as_tensor(np.asarray(bg, dtype=np.float32)).to(model.device)
    cols = None if tcol is None else torch.as_tensor(np.asarray(tcol, dtype=np.int64)).to(model.device)

    def v(Xm):
        Y = model.impute(Xm, [i, t]).double()
        return Y if cols is None else Y[:, cols]
    out = None
    for o in np.asarray(orders):
        Xm = Xd.clone()
        prev = v(Xm)
        if out is None:
            out = torch.zeros(prev.shape[0], len(feat), prev.shape[1], dtype=torch.float64, device=prev.device)
        for k in o:
            f = int(feat[int(k)])
            Xm[:, f] = bgd[f]
            cur = v(Xm)
            out[:, int(k)] += prev - cur
            prev = cur
    return (out / len(orders)).cpu().numpy()


def err(values, ref):
    """The issue's error measure: max |values - ref| / max |ref|."""
    return float(np.abs(np.asarray(values) - ref).max() / np.abs(ref).max())

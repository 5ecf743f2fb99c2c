"""Feature impact on the MI355X: which input features of one modality drive the values imputed for another (the use the reference
covers with `evaluate_impact`; the reference source is not available, so the quantity is BUILD-DEFINED here).

    feature_impact(model, X, i, t, background, features, measured)   {'impact' [F], 'per_target' [F, d_t], 'baseline' [d_t] or None}
    plan(n_cells, d_from, d_to, n_features, max_workspace)           the cell chunks and feature groups (host arithmetic only)

Definition.  X [N, d_i] are standardised cells of modality i, bg [d_i] a background vector in the same space, Y = impute(X, [i, t])
the network's eval-mode output in modality t's standardised space and Y^(f) the same with column f of X set to bg[f].  With a
reference matrix R [N, d_t] -- Y itself ("sensitivity"), or the standardised measured values of modality t ("error under occlusion") --

    per_target[k, j] = 1/N sum_c (Y^(feat[k])[c, j] - R[c, j])^2        impact[k] = mean_j per_target[k, j]
    baseline[j]      = 1/N sum_c (Y[c, j] - R[c, j])^2                  (with measured values only: the caller forms the drop)

Route.  The first encoder layer is linear, so occluding feature f changes a cell's pre-activation H = W0 x + b by the rank-one term
(bg_f - x_f) W0[:, f].  Per cell chunk the d -> 2d product is taken ONCE; per group of features `jamie_occlusion_rows` writes the
first hidden activation of every (feature, cell) pair from H, the existing eval GEMMs carry those g n rows through the rest of the
encoder, the mu head and the decoder, and `jamie_impact_accumulate` adds the squared differences in fp64 in a fixed order.  The
[cells x features, d_i] modified inputs are never built and the [features, cells, d_t] outputs never leave the device.  Kernels:
csrc/impact.hip (include/jamie_hip.h, "Feature impact on the device").
"""
import numpy as np
import torch

from . import _native as nv
from .model import BN_EPS, LRELU_SLOPE

GROUP = 8               # features whose columns of W0 a lane of jamie_occlusion_rows holds (csrc/impact.hip OCC_G)
CELL_CHUNK = 8192       # most cells per pass
MAX_GROUP = 32768       # most features per pass
ROW_BLOCK = nv.IMPACT_ROWS

_MODEL_PARTS = ('_linear', '_lin_bn_act', '_encode_eval', '_mu_eval', '_decode_eval', 'p', 'bn', 'input_dim')


def plan(n_cells, d_from, d_to, n_features, max_workspace=1 << 30):
    """The schedule of feature_impact: `n` cells per chunk, `g` features per group, `chunks` [(first cell, cells)], `groups`
    [(first position in the feature list, features)], `rows` = g n and `workspace` = the bytes of the widest activation
    ([g n, 2 max(d_from, d_to)] fp32), which `max_workspace` caps.  (A layer's input and output are alive together, so the peak above
    the inputs is about twice that.)  A chunk first shrinks until GROUP features fit beside each other -- a row of H is read once per
    GROUP features -- and the group then takes what the cap leaves.  ValueError when one feature of one cell does not fit."""
    n_cells, d_from, d_to, n_features, max_workspace = int(n_cells), int(d_from), int(d_to), int(n_features), int(max_workspace)
    if n_cells < 1 or d_from < 1 or d_to < 1 or n_features < 1:
        raise ValueError(f'feature impact needs >= 1 cell, input feature, target feature and occluded feature, got {n_cells} cells, '
                         f'd_from = {d_from}, d_to = {d_to}, {n_features} features')
    row_bytes = 4 * 2 * max(d_from, d_to)
    rows = min(max_workspace // row_bytes, (1 << 31) - 2)
    if rows < 1:
        raise ValueError(f'max_workspace = {max_workspace} bytes is less than the {row_bytes} one occluded cell needs')
    n = min(n_cells, CELL_CHUNK, max(1, rows // min(n_features, GROUP)))
    g = min(n_features, rows // n, MAX_GROUP)
    return {'n': n, 'g': g, 'rows': g * n, 'workspace': g * n * row_bytes,
            'chunks': [(c0, min(n, n_cells - c0)) for c0 in range(0, n_cells, n)],
            'groups': [(k0, min(g, n_features - k0)) for k0 in range(0, n_features, g)]}


def _shape(X):
    return tuple(X.shape) if hasattr(X, 'shape') else np.asarray(X).shape


def _finite(X):
    if hasattr(X, 'tocsr'):                                    # scipy sparse: the stored values
        return bool(np.isfinite(X.tocsr().data).all())
    if torch.is_tensor(X):
        return bool(torch.isfinite(X).all())
    return bool(np.isfinite(np.asarray(X)).all())


def _check_model(model, from_modality, to_modality):
    if not all(hasattr(model, a) for a in _MODEL_PARTS):
        raise ValueError('feature_impact needs a jamie_amd.edModelVar (its eval GEMM paths _linear, _lin_bn_act, _mu_eval, '
                         f'_decode_eval), got {type(model).__name__}')
    M = len(model.input_dim)
    i, t = int(from_modality), int(to_modality)
    if not (0 <= i < M and 0 <= t < M):
        raise ValueError(f'feature_impact: modalities must lie in [0, {M}), got from {from_modality} to {to_modality}')
    return i, t


def check_arguments(model, X, from_modality, to_modality, background=None, features=None, measured=None, max_workspace=1 << 30):
    """Everything feature_impact refuses, on the host and before the GPU is touched: (i, t, N, features int32 [F], plan)."""
    i, t = _check_model(model, from_modality, to_modality)
    d_i, d_t = int(model.input_dim[i]), int(model.input_dim[t])
    sx = _shape(X)
    if len(sx) != 2:
        raise ValueError(f'feature_impact: cells must be 2-D [cells, features], got shape {sx}')
    if sx[0] < 1 or sx[1] != d_i:
        raise ValueError(f'feature_impact: modality {i} has {d_i} features and >= 1 cell is needed, got shape {sx}')
    if not _finite(X):
        raise ValueError('feature_impact: the cells contain NaN or infinity')
    if background is not None:
        if _shape(background) != (d_i,):
            raise ValueError(f'feature_impact: background must be one value per feature [{d_i}], got shape {_shape(background)}')
        if not _finite(background):
            raise ValueError('feature_impact: background contains NaN or infinity')
    if measured is not None:
        if _shape(measured) != (sx[0], d_t):
            raise ValueError(f'feature_impact: measured values must have shape {(sx[0], d_t)}, got {_shape(measured)}')
        if not _finite(measured):
            raise ValueError('feature_impact: the measured values contain NaN or infinity')
    feat = nv.check_features(np.arange(d_i) if features is None else features, d_i, 'feature_impact')
    pd = getattr(model, 'pdims', model.input_dim)
    return i, t, sx[0], feat, plan(sx[0], pd[i], pd[t], len(feat), max_workspace)


def _to_device(X, dev):
    t = X if torch.is_tensor(X) else torch.from_numpy(np.ascontiguousarray(np.asarray(X)))
    return t.to(dev, torch.float32).contiguous()


def feature_impact(model, X, from_modality, to_modality, background=None, features=None, measured=None, max_workspace=1 << 30,
                   device='cuda'):
    """Occlusion impact of the input features `features` (default: all; any order, repeats allowed) of modality `from_modality` on
    the values imputed for `to_modality`.  X [N, d_i]: standardised cells (numpy or tensor); `background` [d_i]: what an occluded
    feature is set to, in the same space (default 0, the fitted mean); `measured` [N, d_t]: standardised measured values of the
    target modality -- the reference matrix is then these instead of the un-occluded imputation, and `baseline` is returned.
    `max_workspace`: cap in bytes on the widest activation of a pass (see `plan`).  Returns float64 numpy: 'impact' [F],
    'per_target' [F, d_t], 'baseline' [d_t] or None."""
    i, t, N, feat, p = check_arguments(model, X, from_modality, to_modality, background, features, measured, max_workspace)
    nv.require_gpu()
    dev = torch.device(getattr(model, 'device', device))
    d_i, d_t = int(model.input_dim[i]), int(model.input_dim[t])
    Xd = _to_device(X, dev)
    bg = torch.zeros(d_i, device=dev) if background is None else _to_device(background, dev)
    Rd = None if measured is None else _to_device(measured, dev)
    W0, b0 = model.p[f'm{i}.enc0.W'], model.p[f'm{i}.enc0.b']
    bn0 = tuple(model.bn[f'm{i}.bn0.{k}'] for k in ('mean', 'var')) + tuple(model.p[f'm{i}.bn0.{k}'] for k in ('g', 'b'))
    h = W0.shape[0]
    F, n, g = len(feat), p['n'], p['g']
    feat_dev = torch.from_numpy(feat).to(dev)
    acc = torch.zeros(F, d_t, dtype=torch.float64, device=dev)
    base = None if Rd is None else torch.zeros(1, d_t, dtype=torch.float64, device=dev)
    A0 = torch.empty(g * n, h, device=dev)
    ws_occ = torch.empty(nv.occlusion_workspace(g, h), dtype=torch.uint8, device=dev)
    ws_acc = torch.empty(nv.impact_accumulate_workspace(n, d_t, g), dtype=torch.uint8, device=dev)
    for c0, nc in p['chunks']:
        x = Xd[c0:c0 + nc]
        H = model._linear(x, W0, b0)                           # W0 x + b before BatchNorm: once per chunk
        Ybase = model._decode_eval(t, model._mu_eval(i, model._encode_eval(i, x)))
        R = Ybase if Rd is None else Rd[c0:c0 + nc]
        if base is not None:
            nv.impact_accumulate(Ybase, R, base, ws_acc, dt=d_t)
        for k0, gc in p['groups']:
            a0 = A0[:gc * nc]
            nv.occlusion_rows(H, x, bg, W0, feat[k0:k0 + gc], bn0, a0, ws_occ, h=h, d=d_i, eps=BN_EPS, slope=LRELU_SLOPE,
                              feat_dev=feat_dev[k0:k0 + gc])
            Yf = model._decode_eval(t, model._mu_eval(i, model._lin_bn_act(i, a0, 'enc1', 'bn1')))
            nv.impact_accumulate(Yf, R, acc[k0:k0 + gc], ws_acc, dt=d_t)
            del Yf
    per_target = acc.cpu().numpy() / float(N)
    return {'impact': per_target.mean(axis=1), 'per_target': per_target,
            'baseline': None if base is None else base.cpu().numpy()[0] / float(N)}

"""Shapley attributions on the MI355X: how much each input feature of one modality contributes to the values imputed for another,
per cell, by permutation walks (the use the reference's notebooks cover with SHAP; BUILD-DEFINED here).

    shapley_values(model, X, i, t, background, features, targets, orders)   {'values' [N, F, T] or None, 'mean_abs', 'mean' [F, T], ...}
    plan(n_cells, d_from, d_to, F, T, max_workspace, max_accumulator)       the cell chunks and step segments (host arithmetic only)
    draw_orders(F, n_permutations, antithetic, seed)                        the orders the facade draws

Definition.  X [N, d_i] are standardised cells of modality i, bg [d_i] a background in the same space, feat [F] DISTINCT input
features (the players), tcol [T] distinct target columns of modality t.  For cell c and a coalition S of players, v_c(S) [T] is the
eval-mode imputation `model.impute(., [i, t])` of the cell with every player NOT in S set to its background; the other features keep
the cell's values.  An order o [F] (a permutation of 0 .. F-1, positions in `feat`) is walked as removals: S_0 = all players,
S_m = S_{m-1} without player o[m-1], and player o[m-1] receives v_c(S_{m-1}) - v_c(S_m) -- the permutation-sampling estimator for
the adding order reverse(o); averaged over all F! orders it is the exact Shapley value.  One order is shared by all cells of a pass
(unbiased per cell).  With P orders,

    values[c, k, j] = mean over the orders of player k's contribution to target tcol[j]       (float64)
    mean_abs[k, j]  = 1/N sum_c |values[c, k, j]|      mean[k, j] = 1/N sum_c values[c, k, j]      importance[k] = mean_j mean_abs[k, j]

Route.  The first encoder layer is linear, so a step of a walk changes a cell's pre-activation H = W0 x + b by one rank-one term.
Per cell chunk the d -> 2d product is taken ONCE; per order H is copied into a state, and per segment of g steps
`jamie_shapley_walk_rows` writes the first hidden activation of the g + 1 prefixes of every cell from the state (and leaves the
state at the segment's end), the existing eval GEMMs carry those (g + 1) n rows through the rest of the encoder, the mu head and the
decoder, and `jamie_shapley_accumulate` adds the differences of consecutive rows onto a float64 accumulator [n, F, T].
`jamie_shapley_summarise` reduces the chunk over its cells in a fixed order.  The masked inputs never exist.  Kernels:
csrc/shapley.hip (include/jamie_hip.h, "Shapley attributions on the device").
"""
import numpy as np
import torch

from . import _native as nv
from .impact import _MODEL_PARTS, _finite, _shape, _to_device
from .model import BN_EPS, LRELU_SLOPE

GROUP = 8               # rows of W0^T a lane of jamie_shapley_walk_rows holds ahead of its chain (csrc/shapley.hip WALK_G)
CELL_CHUNK = 8192       # most cells per chunk
MAX_SEGMENT = 32768     # most steps per segment
MAX_HOST_VALUES = 1 << 32   # most bytes of `values` [N, F, T] float64 that return_values brings to the host


def _check_model(model, from_modality, to_modality):
    if not all(hasattr(model, a) for a in _MODEL_PARTS):
        raise ValueError('shapley_values needs a jamie_amd.edModelVar (its eval GEMM paths _linear, _lin_bn_act, _mu_eval, '
                         f'_decode_eval), got {type(model).__name__}')
    M = len(model.input_dim)
    i, t = int(from_modality), int(to_modality)
    if not (0 <= i < M and 0 <= t < M):
        raise ValueError(f'shapley_values: modalities must lie in [0, {M}), got from {from_modality} to {to_modality}')
    return i, t


def plan(n_cells, d_from, d_to, n_players, n_targets, max_workspace=1 << 30, max_accumulator=1 << 30):
    """The schedule of shapley_values: `n` cells per chunk, `g` steps per segment, `chunks` [(first cell, cells)], `segments`
    [(first step, steps)], `rows` = (g + 1) n, `workspace` = the bytes of the widest activation ([(g + 1) n, 2 max(d_from, d_to)]
    fp32), which `max_workspace` caps, and `accumulator` = 8 n F T bytes of float64 contributions, which `max_accumulator` caps.
    A chunk is at most CELL_CHUNK cells and what the accumulator cap admits, and shrinks until GROUP steps and the incoming row fit
    beside each other (a segment re-emits its incoming row: it pushes g + 1 rows for g steps); the segment then takes what the
    workspace cap leaves.  ValueError when one cell does not fit either cap."""
    n_cells, d_from, d_to, F, T = int(n_cells), int(d_from), int(d_to), int(n_players), int(n_targets)
    max_workspace, max_accumulator = int(max_workspace), int(max_accumulator)
    if n_cells < 1 or d_from < 1 or d_to < 1 or F < 1 or T < 1:
        raise ValueError(f'shapley values need >= 1 cell, input feature, target feature, player and target, got {n_cells} cells, '
                         f'd_from = {d_from}, d_to = {d_to}, {F} players, {T} targets')
    row_bytes = 4 * 2 * max(d_from, d_to)
    rows = min(max_workspace // row_bytes, (1 << 31) - 2)
    if rows < 2:
        raise ValueError(f'max_workspace = {max_workspace} bytes is less than the {2 * row_bytes} one step of one cell needs')
    acc_cells = max_accumulator // (8 * F * T)
    if acc_cells < 1:
        raise ValueError(f'max_accumulator = {max_accumulator} bytes is less than the {8 * F * T} one cell needs '
                         f'({F} players x {T} targets in float64)')
    n = min(n_cells, CELL_CHUNK, acc_cells, max(1, rows // (min(F, GROUP) + 1)))
    g = min(F, rows // n - 1, MAX_SEGMENT)
    return {'n': n, 'g': g, 'rows': (g + 1) * n, 'workspace': (g + 1) * n * row_bytes, 'accumulator': 8 * n * F * T,
            'chunks': [(c0, min(n, n_cells - c0)) for c0 in range(0, n_cells, n)],
            'segments': [(m0, min(g, F - m0)) for m0 in range(0, F, g)]}


def draw_orders(n_players, n_permutations=16, antithetic=True, seed=0):
    """int32 [P, F]: `n_permutations` orders drawn with np.random.default_rng(seed); with `antithetic` each is followed by its
    reverse (P = 2 n_permutations)."""
    F, K = int(n_players), int(n_permutations)
    if F < 1 or K < 1:
        raise ValueError(f'shapley_values: >= 1 player and >= 1 permutation are needed, got {F} players, n_permutations = {K}')
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(K):
        o = rng.permutation(F).astype(np.int32)
        out.append(o)
        if antithetic:
            out.append(o[::-1])
    return np.ascontiguousarray(np.stack(out), dtype=np.int32)


def check_orders(orders, n_players):
    """`orders` as contiguous int32 [P >= 1, F], every row a permutation of range(F), or ValueError."""
    F = int(n_players)
    a = np.asarray(orders)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != F or a.dtype.kind not in 'iu':
        raise ValueError(f'shapley_values: orders must be integers of shape [P >= 1, {F}], got shape {a.shape} and dtype {a.dtype}')
    if not np.array_equal(np.sort(a, axis=1), np.broadcast_to(np.arange(F), a.shape)):
        raise ValueError(f'shapley_values: every row of orders must be a permutation of range({F})')
    return np.ascontiguousarray(a, dtype=np.int32)


def check_arguments(model, X, from_modality, to_modality, background=None, features=None, targets=None, orders=None,
                    max_workspace=1 << 30, max_accumulator=1 << 30, return_values=False):
    """Everything shapley_values refuses, on the host and before the GPU is touched:
    (i, t, N, features int32 [F], targets int32 [T] or None for all, orders int32 [P, F], plan)."""
    who = 'shapley_values'
    i, t = _check_model(model, from_modality, to_modality)
    d_i, d_t = int(model.input_dim[i]), int(model.input_dim[t])
    sx = _shape(X)
    if len(sx) != 2:
        raise ValueError(f'{who}: cells must be 2-D [cells, features], got shape {sx}')
    if sx[0] < 1 or sx[1] != d_i:
        raise ValueError(f'{who}: modality {i} has {d_i} features and >= 1 cell is needed, got shape {sx}')
    if not _finite(X):
        raise ValueError(f'{who}: the cells contain NaN or infinity')
    if background is not None:
        if _shape(background) != (d_i,):
            raise ValueError(f'{who}: background must be one value per feature [{d_i}], got shape {_shape(background)}')
        if not _finite(background):
            raise ValueError(f'{who}: background contains NaN or infinity')
    feat = nv.check_distinct(np.arange(d_i) if features is None else features, d_i, who, 'the features (players)')
    tcol = None if targets is None else nv.check_distinct(targets, d_t, who, 'the targets')
    if orders is None:
        raise ValueError(f'{who}: orders [P, F] are needed (draw_orders)')
    orders = check_orders(orders, len(feat))
    F, T = len(feat), d_t if tcol is None else len(tcol)
    pd = getattr(model, 'pdims', model.input_dim)
    p = plan(sx[0], pd[i], pd[t], F, T, max_workspace, max_accumulator)
    if return_values and 8 * sx[0] * F * T > MAX_HOST_VALUES:
        raise ValueError(f'{who}: return_values would bring {8 * sx[0] * F * T} bytes [{sx[0]}, {F}, {T}] float64 to the host, more '
                         f'than {MAX_HOST_VALUES}; choose fewer cells, features or targets')
    return i, t, sx[0], feat, tcol, orders, p


def shapley_values(model, X, from_modality, to_modality, background=None, features=None, targets=None, orders=None,
                   max_workspace=1 << 30, max_accumulator=1 << 30, return_values=False, device='cuda'):
    """Shapley attributions of the input features `features` (default: all; distinct, any order) of modality `from_modality` for the
    columns `targets` (default: all; distinct, any order) of the values imputed for `to_modality`, estimated over the walks
    `orders` [P, F] (permutations of range(F), positions in `features`; see `draw_orders`).  X [N, d_i]: standardised cells (numpy or
    tensor); `background` [d_i]: what a removed feature is set to, in the same space (default 0, the fitted mean).
    `max_workspace`, `max_accumulator`: caps in bytes on the widest activation of a pass and on the float64 contributions of a cell
    chunk (see `plan`).  Returns float64 numpy: 'values' [N, F, T] (None unless `return_values`), 'mean_abs' [F, T], 'mean' [F, T],
    'importance' [F], and 'orders' [P, F] int32."""
    i, t, N, feat, tcol, orders, p = check_arguments(model, X, from_modality, to_modality, background, features, targets, orders,
                                                     max_workspace, max_accumulator, return_values)
    nv.require_gpu()
    dev = torch.device(getattr(model, 'device', device))
    d_i, d_t = int(model.input_dim[i]), int(model.input_dim[t])
    Xd = _to_device(X, dev)
    bg = torch.zeros(d_i, device=dev) if background is None else _to_device(background, dev)
    W0, b0 = model.p[f'm{i}.enc0.W'], model.p[f'm{i}.enc0.b']
    bn0 = tuple(model.bn[f'm{i}.bn0.{k}'] for k in ('mean', 'var')) + tuple(model.p[f'm{i}.bn0.{k}'] for k in ('g', 'b'))
    h = W0.shape[0]
    F, T, P, n, g = len(feat), (d_t if tcol is None else len(tcol)), len(orders), p['n'], p['g']
    walk_feat = np.ascontiguousarray(feat[orders])             # [P, F]: the feature removed at every step of every order
    walk_feat_dev, orders_dev = torch.from_numpy(walk_feat).to(dev), torch.from_numpy(orders).to(dev)
    tcol_dev = None if tcol is None else torch.from_numpy(tcol).to(dev)
    phi = torch.empty(n, F, T, dtype=torch.float64, device=dev)
    sum_abs = torch.zeros(F, T, dtype=torch.float64, device=dev)
    total = torch.zeros(F, T, dtype=torch.float64, device=dev)
    state = torch.empty(n, h, device=dev)
    A0 = torch.empty((g + 1) * n, h, device=dev)
    ws_walk = torch.empty(nv.shapley_walk_workspace(g, h), dtype=torch.uint8, device=dev)
    ws_sum = torch.empty(nv.shapley_summarise_workspace(n, F * T), dtype=torch.uint8, device=dev)
    values = np.empty((N, F, T), np.float64) if return_values else None
    for c0, nc in p['chunks']:
        x = Xd[c0:c0 + nc]
        H = model._linear(x, W0, b0)                           # W0 x + b before BatchNorm: once per chunk
        ph, st = phi[:nc], state[:nc]
        ph.zero_()
        for q in range(P):
            st.copy_(H)
            for m0, gc in p['segments']:
                a0 = A0[:(gc + 1) * nc]
                nv.shapley_walk_rows(st, x, bg, W0, walk_feat[q, m0:m0 + gc], bn0, a0, ws_walk, h=h, d=d_i, eps=BN_EPS,
                                     slope=LRELU_SLOPE, feat_dev=walk_feat_dev[q, m0:m0 + gc])
                Y = model._decode_eval(t, model._mu_eval(i, model._lin_bn_act(i, a0, 'enc1', 'bn1')))
                nv.shapley_accumulate(Y, orders[q, m0:m0 + gc], ph, tcol=tcol, dt=d_t, pos_dev=orders_dev[q, m0:m0 + gc],
                                      tcol_dev=tcol_dev)
                del Y
        nv.shapley_summarise(ph, sum_abs, total, ws_sum)
        if values is not None:
            values[c0:c0 + nc] = ph.cpu().numpy() / float(P)
    mean_abs = sum_abs.cpu().numpy() / (float(P) * float(N))
    return {'values': values, 'mean_abs': mean_abs, 'mean': total.cpu().numpy() / (float(P) * float(N)),
            'importance': mean_abs.mean(axis=1), 'orders': orders}

"""Shared by test_host_silhouette.py and test_hip_silhouette.py: inputs, the float64 reference, the error bound of DESIGN.md §16
and a numpy fp32 restatement of the device reduction."""
import functools

import numpy as np

U = 2.0 ** -24
CLASS_SIZES = (1, 2, 127, 128, 129, 13)        # 400 rows: boundaries inside a tile, exactly one tile, one row past a tile
DIMS = (1, 3, 32, 33, 64)
KINDS = ('gaussian', 'clustered', 'offset')


def gamma(L):
    """Relative error bound of every S[i, c]: the q chain (L + 2) u, halved by the square root, + u for the square root, + 7 u
    for the fp32 partial of 8 columns."""
    return (L / 2 + 9) * U


def width_bound(L):
    """Absolute error bound of a silhouette width: s = 1 - a / b or b / a - 1 with relative error at most gamma on a and on b."""
    g = gamma(L)
    return 2 * g / (1 - g)


def class_codes(sizes=CLASS_SIZES, seed=0):
    """One code per row, shuffled: class c has sizes[c] rows."""
    codes = np.repeat(np.arange(len(sizes)), sizes)
    return np.random.default_rng(seed).permutation(codes)


@functools.lru_cache(maxsize=None)
def data(kind, N, L, seed=0):
    """fp32 [N, L] and codes [N] with CLASS_SIZES (N = 400): Gaussian; clusters around one centre per class; Gaussian offset by 50
    (distances small against the coordinates)."""
    rng = np.random.default_rng(1000 * seed + 10 * L + KINDS.index(kind))
    codes = class_codes(seed=seed + L)
    assert len(codes) == N
    X = rng.standard_normal((N, L))
    if kind == 'clustered':
        X = 0.3 * X + 2.0 * rng.standard_normal((len(CLASS_SIZES), L))[codes]
    elif kind == 'offset':
        X = X + 50.0
    X = X.astype(np.float32)
    X.setflags(write=False)
    codes.setflags(write=False)
    return X, codes


def reference_sums(Q, R, codes, n_classes):
    """float64 by direct difference: S[i, c] = sum over the rows j of R with code c of |Q_i - R_j|."""
    from scipy.spatial.distance import cdist
    d = cdist(np.asarray(Q, dtype=np.float64), np.asarray(R, dtype=np.float64))
    S = np.zeros((len(Q), n_classes))
    for c in range(n_classes):
        S[:, c] = d[:, codes == c].sum(axis=1)
    return S


def widths_from_sums(S, counts, own, win0=None, wlen=None):
    """The definition of jamie_silhouette_widths, one cell at a time."""
    N, C = S.shape
    wlen = C if wlen is None else wlen
    out = np.empty(N)
    for i in range(N):
        w0 = 0 if win0 is None else int(win0[i])
        others = [S[i, c] / counts[c] for c in range(w0, min(w0 + wlen, C)) if c != own[i] and counts[c] > 0]
        if not others:
            out[i] = np.nan
        elif counts[own[i]] == 1:
            out[i] = 0.0
        else:
            a, b = S[i, own[i]] / (counts[own[i]] - 1), min(others)
            out[i] = 0.0 if max(a, b) == 0 else (b - a) / max(a, b)
    return out


def restated_sums(Q, R, codes, n_classes, seg_tiles=1 << 30):
    """The device reduction in numpy: R in class order (stable); q by the fp32 chain t = a - b, q = fma(t, t, q) in ascending
    feature order; sqrt in fp32; per 128-row tile of a class a thread tx adds its 8 columns (m * 64 + tx * 4 + k) in fp32 in
    ascending order; fp64 accumulators per tx over the tiles of a segment; the 16 tx by the xor tree 8, 4, 2, 1; the segments in
    order."""
    Q, R = np.asarray(Q, dtype=np.float32), np.asarray(R, dtype=np.float32)
    order = np.argsort(codes, kind='stable')
    Rs, cs = R[order], np.asarray(codes)[order]
    q = np.zeros((len(Q), len(Rs)), dtype=np.float32)
    for c in range(Q.shape[1]):
        t = (Q[:, c][:, None] - Rs[:, c][None, :]).astype(np.float32)
        q = (q.astype(np.float64) + t.astype(np.float64) * t.astype(np.float64)).astype(np.float32)      # fma: one rounding
    d = np.sqrt(q)
    assert d.dtype == np.float32
    S = np.zeros((len(Q), n_classes))
    for c in range(n_classes):
        dc = d[:, cs == c]
        n = dc.shape[1]
        tiles = (n + 127) // 128
        dc = np.concatenate([dc, np.zeros((len(Q), tiles * 128 - n), np.float32)], axis=1).reshape(len(Q), tiles, 2, 16, 4)
        total = np.zeros(len(Q))
        for t0 in range(0, tiles, seg_tiles):
            acc = np.zeros((len(Q), 16))
            for t in range(t0, min(t0 + seg_tiles, tiles)):
                p = dc[:, t, 0, :, 0].copy()
                for m, k in [(0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3)]:
                    p = (p + dc[:, t, m, :, k]).astype(np.float32)
                acc = acc + p.astype(np.float64)
            for x in (8, 4, 2, 1):
                acc = acc + acc[:, np.arange(16) ^ x]
            total = total + acc[:, 0]
        S[:, c] = total
    return S


@functools.lru_cache(maxsize=None)
def two_by_three(L=8, seed=3):
    """2 modalities x 3 labels, label 'c' missing from the second modality: (e0, l0, e1, l1), fp32-representable float64."""
    rng = np.random.default_rng(seed)
    centres = 3.0 * rng.standard_normal((3, L))
    l0 = np.array(['a'] * 70 + ['b'] * 60 + ['c'] * 30)
    l1 = np.array(['b'] * 80 + ['a'] * 50)
    names = {'a': 0, 'b': 1, 'c': 2}
    e0 = centres[[names[x] for x in l0]] + rng.standard_normal((len(l0), L))
    e1 = centres[[names[x] for x in l1]] + rng.standard_normal((len(l1), L)) + 0.4
    e0, e1 = e0.astype(np.float32).astype(np.float64), e1.astype(np.float32).astype(np.float64)
    p0, p1 = rng.permutation(len(l0)), rng.permutation(len(l1))
    out = (e0[p0], l0[p0], e1[p1], l1[p1])
    for x in out:
        x.setflags(write=False)
    return out


def silhouette_by_loops(embeddings, labels):
    """The definition of JAMIE.test_silhouette in plain loops over float64 distances."""
    M = len(embeddings)
    X = np.concatenate([np.asarray(e, dtype=np.float64) for e in embeddings])
    lab = np.concatenate(labels)
    mod = np.concatenate([[m] * len(e) for m, e in enumerate(embeddings)])
    N = len(X)
    d = np.array([[np.sqrt(((X[i] - X[j]) ** 2).sum()) for j in range(N)] for i in range(N)])
    names = sorted(set(lab.tolist()))

    def width(i, cluster, cells):
        """silhouette of cell i with clusters `cluster` among `cells`"""
        mine = [j for j in cells if cluster[j] == cluster[i]]
        rest = sorted(set(cluster[j] for j in cells) - {cluster[i]})
        if len(mine) == 1:
            return 0.0
        a = sum(d[i, j] for j in mine) / (len(mine) - 1)
        b = min(sum(d[i, j] for j in cells if cluster[j] == o) / sum(1 for j in cells if cluster[j] == o) for o in rest)
        return 0.0 if max(a, b) == 0 else (b - a) / max(a, b)

    every = list(range(N))
    label_widths = np.array([width(i, lab, every) for i in every])
    per_label = np.full(len(names), np.nan)
    for t, name in enumerate(names):
        cells = [i for i in every if lab[i] == name]
        if len(set(mod[i] for i in cells)) >= 2:
            per_label[t] = np.mean([1 - abs(width(i, mod, cells)) for i in cells])
    dist = np.array([[np.mean([d[i, j] for i in every if lab[i] == s for j in every if lab[j] == t]) for t in names] for s in names])
    return {'label_asw': float(label_widths.mean()), 'label_widths': label_widths,
            'modality_asw': float(np.nanmean(per_label)), 'modality_asw_per_label': per_label, 'label_distance': dist,
            'labels': np.array(names)}

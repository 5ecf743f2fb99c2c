"""Shared by tests/test_host_tsne.py and tests/test_hip_tsne.py: inputs, float64 references and the numpy restatement of what
csrc/tsne.hip computes."""
import functools

import numpy as np

import lisi_util as lu

# Relative tolerance of a device sum of the gradient (A_i, R_i per coordinate, z_i, Z, KL) against float64 numpy on the same fp32
# layout and the same stored P, relative to the float64 sum of the MAGNITUDES of the terms (forces cancel: the result is no
# yardstick).  The chain: dx, dy one fp32 rounding each; d = fma(dx, dx, fma(dy, dy, 1)) two; w = 1 / d after the Newton step one;
# w * w one; the fma into the partial one: a term is good to about 8 x 2^-24 of its magnitude in the worst case, and the fp32
# partial over a run of 32 columns adds up to 31 x 2^-24 of the run's magnitudes in the worst case, 39 x 2^-24 = 2.3e-6 together.
# Roundings do not conspire like that: the numpy restatement of the design (test_host_tsne.py::test_design_restated) shows
# 2.6e-7 at most over the states of the GPU test (three layouts at each size of SHAPES, and the blobs), and the asserted bound
# is capped at 4 x that.
GRAD_TOL = 7.5e-7
RUN = 32               # columns per fp32 partial sum of the repulsion kernel
NEAR_BRANCH = 1e-11    # a solve whose trace comes this close to a branch is left out of the device comparison
NEAR_BRANCH_CAP = 0.005

# pooled N -> ((cells per modality), L, K, perplexity): below one tile, one past a tile, several segments at seg_rows = 128, not a
# multiple of anything, and 2600: the repulsion kernel's own geometry (1024 rows per workgroup, 512 columns per staged chunk) needs
# more than 1024 cells before there is a second block of rows, a chunk without rows of the workgroup, or (with SEG_ROWS_LONG) a
# segment of several chunks with the next chunk's load in flight and a tail chunk
SHAPES = {8: ((5, 3), 4, 7, 2.0), 130: ((70, 60), 8, 30, 10.0), 257: ((129, 128), 16, 45, 15.0), 600: ((350, 250), 32, 90, 30.0),
          1000: ((1000,), 3, 128, 40.0), 2600: ((1400, 1200), 8, 30, 10.0)}
SEG_ROWS_LONG = (1280, 2688)      # at N = 2600: segments of 1280, 1280 and 40 columns; one segment of five chunks and a tail of 40


def seg_rows_of(N):
    """The seg_rows the gradient is compared at."""
    return (0, 128, 256) + (SEG_ROWS_LONG if N > 1024 else ())


def blobs(seed=0):
    """Four gaussian blobs of 100 cells, L = 8, sd 1, centres 10 apart, as two embeddings of 200 cells: (embeddings, labels)."""
    rng = np.random.default_rng(seed)
    centres = np.zeros((4, 8))
    centres[np.arange(4), np.arange(4)] = 10.0 / np.sqrt(2.0)
    lab = np.repeat(np.arange(4), 100)
    X = (centres[lab] + rng.standard_normal((400, 8))).astype(np.float32)
    order = rng.permutation(400)
    X, lab = X[order], lab[order]
    return [X[:200], X[200:]], [lab[:200], lab[200:]]


def affinity_reference(dist, perplexity):
    """The float64 loop of DESIGN.md §19 step 2 over all cells: (C [N, K], beta, tries, entropy, margin); margin the smallest of
    | |Hdiff| - 1e-5 | and |Hdiff| seen in the trace: where a last-bit difference could change a branch."""
    dist = np.asarray(dist, np.float64)
    log_u = np.log(perplexity)
    N, K = dist.shape
    C, beta_out, tries, ent, margin = np.empty((N, K)), np.empty(N), np.empty(N, np.int64), np.empty(N), np.empty(N)
    for i in range(N):
        e = dist[i] ** 2 - dist[i, 0] ** 2
        beta, bmin, bmax, t, m = 1.0, -np.inf, np.inf, 0, np.inf
        while True:
            P = np.exp(-beta * e)
            s = P.sum()
            H = np.log(s) + beta * np.sum(e * P) / s
            diff = H - log_u
            m = min(m, abs(abs(diff) - 1e-5), abs(diff))
            if not (abs(diff) > 1e-5 and t < 100):
                break
            if diff > 0:
                bmin = beta
                beta = beta * 2 if bmax == np.inf else (beta + bmax) / 2
            else:
                bmax = beta
                beta = beta / 2 if bmin == -np.inf else (beta + bmin) / 2
            t += 1
        C[i], beta_out[i], tries[i], ent[i], margin[i] = P / s, beta, t, H, m
    return C, beta_out, tries, ent, margin


def joint_reference(idx, C):
    """(C + C^T) / (2N) as scipy CSR in float64 with sorted indices, from lists idx [N, K] and conditional affinities C [N, K]."""
    from scipy.sparse import csr_matrix
    N, K = idx.shape
    cond = csr_matrix((np.asarray(C, np.float64).reshape(-1), np.asarray(idx).reshape(-1), np.arange(0, N * K + 1, K)), shape=(N, N))
    P = (cond + cond.T) / (2.0 * N)
    P.sort_indices()
    return P


def row_order(idx):
    """The columns of every row of P in the order DESIGN.md §19 fixes: the row's own K in neighbour order, then the cells that list
    it without being listed by it, ascending."""
    N, K = idx.shape
    lists = [set(r.tolist()) for r in idx]
    listed_by = [[] for _ in range(N)]
    for i in range(N):
        for j in idx[i]:
            listed_by[j].append(i)
    return [list(idx[i]) + sorted(s for s in listed_by[i] if s not in lists[i]) for i in range(N)]


def gradient_reference(P, Y):
    """All-float64 sums of the gradient at the fp32 layout Y under scipy CSR P: dict(A, R [N, 2], z [N], Z, KL) and the sums of
    the terms' magnitudes A_mag, R_mag [N, 2], KL_mag."""
    Y = np.asarray(Y, np.float64)
    N = len(Y)
    dx, dy = Y[:, None, 0] - Y[None, :, 0], Y[:, None, 1] - Y[None, :, 1]
    W = 1.0 / (1.0 + dx * dx + dy * dy)
    np.fill_diagonal(W, 0.0)
    W2 = W * W
    Pd = np.asarray(P.todense())
    PW = Pd * W
    out = {'z': W.sum(axis=1), 'Z': float(W.sum()),
           'R': np.stack([(W2 * dx).sum(axis=1), (W2 * dy).sum(axis=1)], axis=1),
           'R_mag': np.stack([(W2 * np.abs(dx)).sum(axis=1), (W2 * np.abs(dy)).sum(axis=1)], axis=1),
           'A': np.stack([(PW * dx).sum(axis=1), (PW * dy).sum(axis=1)], axis=1),
           'A_mag': np.stack([(PW * np.abs(dx)).sum(axis=1), (PW * np.abs(dy)).sum(axis=1)], axis=1)}
    nz = Pd > 0
    terms = Pd[nz] * np.log(Pd[nz] * out['Z'] / W[nz])
    out['KL'], out['KL_mag'] = float(terms.sum()), float(np.abs(terms).sum() + Pd[nz].sum())
    return out


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def restated_gradient(P, Y, seg_rows=0):
    """The device design in numpy: fp32 differences, d = fma(dx, dx, fma(dy, dy, 1)), w = 1 / d rounded once, w * w, the fma into
    an fp32 partial over runs of RUN columns in column order, the partials added in float64; the attraction per entry in fp32
    (p w, then times dx), added in float64.  (An fma is formed in float64 and rounded to fp32.)  Same dict as gradient_reference,
    without the magnitudes."""
    Y = np.asarray(Y, np.float32)
    N = len(Y)
    dx, dy = Y[:, None, 0] - Y[None, :, 0], Y[:, None, 1] - Y[None, :, 1]                    # fp32
    d = _f32(dx.astype(np.float64) ** 2 + _f32(dy.astype(np.float64) ** 2 + 1.0).astype(np.float64))
    w = _f32(1.0 / d.astype(np.float64))
    wz = w.copy()
    np.fill_diagonal(wz, 0.0)
    w2 = (wz * wz).astype(np.float32)
    seg = N if seg_rows == 0 else seg_rows
    z, R = np.zeros(N), np.zeros((N, 2))
    for s0 in range(0, N, seg):
        for c0 in range(s0, min(s0 + seg, N), RUN):
            c1 = min(c0 + RUN, s0 + seg, N)
            pz, px, py = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros(N, np.float32)
            for c in range(c0, c1):
                pz = pz + wz[:, c]
                px = _f32(w2[:, c].astype(np.float64) * dx[:, c] + px)
                py = _f32(w2[:, c].astype(np.float64) * dy[:, c] + py)
            z += pz
            R[:, 0] += px
            R[:, 1] += py
    Pd = np.asarray(P.todense())
    pw = (Pd.astype(np.float32) * w).astype(np.float32)
    A = np.stack([(pw * dx).astype(np.float32).astype(np.float64).sum(axis=1),
                  (pw * dy).astype(np.float32).astype(np.float64).sum(axis=1)], axis=1)
    Z = float(z.sum())
    nz = Pd > 0
    KL = float(np.sum(Pd[nz] * np.log(Pd[nz] * d.astype(np.float64)[nz] * Z)))
    return {'z': z, 'Z': Z, 'R': R, 'A': A, 'KL': KL}


def gradient_errors(got, ref):
    """The largest error of each sum relative to the float64 sum of its terms' magnitudes: dict(A, R, z, Z, KL)."""
    def rel(a, b, mag):
        mag = np.asarray(mag, np.float64)
        err = np.abs(np.asarray(a, np.float64) - b)
        return float(np.max(np.where(mag > 0, err / np.where(mag > 0, mag, 1.0), np.where(err > 0, np.inf, 0.0))))
    return {'A': rel(got['A'], ref['A'], ref['A_mag']), 'R': rel(got['R'], ref['R'], ref['R_mag']), 'z': rel(got['z'], ref['z'], ref['z']),
            'Z': rel(got['Z'], ref['Z'], ref['Z']), 'KL': rel(got['KL'], ref['KL'], ref['KL_mag'])}


def purity(Y, labels, k=10):
    """Mean share of a cell's k nearest other cells in the layout that carry its label."""
    idx, _, _ = lu.knn_reference(np.asarray(Y, np.float64), k)
    labels = np.asarray(labels)
    return float(np.mean(labels[idx] == labels[:, None]))


@functools.lru_cache(maxsize=None)
def shape_case(N):
    """Inputs and float64 references of SHAPES[N], computed once: dict(emb, X, K, u, idx, dist) with the float64 lists."""
    sizes, L, K, u = SHAPES[N]
    emb, _ = lu.mixture(200 + N, 5, L, sizes)
    X = np.concatenate(emb, axis=0)
    idx, dist, _ = lu.knn_reference(X, K)
    return dict(emb=emb, X=X, K=K, u=u, idx=idx, dist=dist)


@functools.lru_cache(maxsize=None)
def host_run(seed, n_iter=300, exaggeration_iter=100):
    """`JAMIE(metrics='host').tsne` of the blobs from the random init of `seed`."""
    from jamie_amd import JAMIE
    emb, _ = blobs()
    return JAMIE(metrics='host').tsne(emb, n_iter=n_iter, exaggeration_iter=exaggeration_iter, init='random', seed=seed, log_every=50)


@functools.lru_cache(maxsize=None)
def spread_layout(N):
    """A spread-out layout of SHAPES[N]: the host route's after 120 iterations (40 of them exaggerated), float32 [N, 2].  Beyond
    1000 cells, where an iteration of the host route takes a second: the PCA scores at a standard deviation of 20."""
    from jamie_amd import JAMIE
    from jamie_amd.tsne import initial_layout
    c = shape_case(N)
    if N > 1000:
        return initial_layout(c['X'], 'pca', 0) * np.float32(2e5)
    out = JAMIE(metrics='host').tsne(c['emb'], perplexity=c['u'], n_neighbors=c['K'], n_iter=120, exaggeration_iter=40, log_every=120)
    return np.concatenate(out['layout'], axis=0)

"""Shared by tests/test_host_spectral.py and tests/test_hip_spectral.py: inputs, the float64 references, the numpy restatement of
what csrc/spectral.hip and jamie_amd/spectral.py compute and the derived checks (a) .. (f) of a solution."""
import functools

import numpy as np

U = 2.0 ** -53
GAP = 1e-3                 # the precondition of the eigenvalue and subspace checks: lambda_k - lambda_(k+1) on the reference
GRAM_ROWS = 512            # rows of a Gram segment (csrc/spectral.hip)
ROWSUM_GROUP = 16          # lanes that own a row in the row sum

# name -> (blobs, cells per blob, L, centre spread, seed, n_neighbors); two modalities each (the halves of a permutation)
BLOBS = {'blobs4': (4, 75, 8, 1.3, 2, 15), 'blobs3': (3, 200, 8, 1.3, 2, 15), 'blobs20': (20, 100, 16, 1.2, 1, 15),
         'cells40': (2, 20, 4, 1.5, 4, 10), 'cells16': (1, 16, 4, 0.0, 5, 16), 'cells17': (1, 17, 4, 0.0, 6, 9)}
# the cases of the eigenvalue and subspace checks -> the k they are run at (k = 13 iterates a block of 32)
SOLVER_CASES = {'blobs4': (3, 11), 'blobs3': (3, 11), 'sheet': (3, 11), 'cells40': (3, 11, 13), 'blobs20': (3, 11), 'apart': (3,)}


@functools.lru_cache(maxsize=None)
def cells(name):
    """(embeddings: a list of fp32 [N_m, L], n_neighbors, coordinate): `coordinate` is the unrolled position of the sheet's cells
    (None elsewhere)."""
    if name == 'sheet':          # 600 cells on a rolled strip: one and a half turns 0.8 apart, 1 wide
        rng = np.random.default_rng(7)
        s = np.sort(rng.uniform(0.0, 1.0, 600))
        phi = 3.0 * np.pi * s
        r = 1.0 + 0.8 * phi / (2.0 * np.pi)
        X = np.stack([r * np.cos(phi), r * np.sin(phi), rng.uniform(0.0, 1.0, 600)], axis=1).astype(np.float32)
        return [X[:350].copy(), X[350:].copy()], 15, s
    if name == 'apart':          # two blobs 100 apart: two components, lambda = 1 twice
        rng = np.random.default_rng(8)
        X = rng.standard_normal((200, 6))
        X[100:, 0] += 100.0
        X = X[rng.permutation(200)].astype(np.float32)
        return [X[:120].copy(), X[120:].copy()], 15, None
    T, per, L, spread, seed, nn = BLOBS[name]
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((T, L)) * spread
    X = (np.repeat(centres, per, axis=0) + rng.standard_normal((T * per, L)))
    X = X[rng.permutation(T * per)].astype(np.float32)
    half = (T * per) // 2
    return [X[:half].copy(), X[half:].copy()], nn, None


@functools.lru_cache(maxsize=None)
def host_graph(name):
    """(rowptr, col, val fp32) of a case's fuzzy graph by the host route's own functions (jamie_amd/jamie.py)."""
    from jamie_amd import jamie as jj
    emb, nn, _ = cells(name)
    order, dist = jj._host_sorted_neighbors(list(emb), nn - 1, 'spectral')
    W, _, _, _ = jj._host_smooth_knn(dist, nn)
    return jj._host_fuzzy_graph(order, W)


def dense_operator(rowptr, col, val, density_normalize):
    """(S [N, N], degree, scale) in float64 numpy from the CSR arrays of a graph: the definition of DESIGN.md §21 step 1."""
    N = len(rowptr) - 1
    A = np.zeros((N, N))
    A[np.repeat(np.arange(N), np.diff(rowptr)), np.asarray(col, np.int64)] = np.asarray(val, np.float64)
    d = A.sum(axis=1)
    if density_normalize:
        inv = 1.0 / d
        d = (A @ inv) * inv
        scale = inv / np.sqrt(d)
    else:
        scale = 1.0 / np.sqrt(d)
    S = scale[:, None] * A * scale[None, :]
    return (S + S.T) / 2.0, d, scale


@functools.lru_cache(maxsize=None)
def reference(name, density_normalize):
    """(lambda descending [N], V [N, N], S, degree, scale) of a case's host graph: `numpy.linalg.eigh` of the dense S."""
    S, d, scale = dense_operator(*host_graph(name), density_normalize)
    w, V = np.linalg.eigh(S)
    return w[::-1].copy(), np.ascontiguousarray(V[:, ::-1]), S, d, scale


# ---- the restatement of the kernels' operation order ----
def restated_rowsum(rowptr, col, val, w=None):
    """jamie_graph_rowsum in numpy: lane l of a row's 16 adds (double)val[e] * w[col[e]] for its entries l, l + 16, ... in order;
    the lanes by the xor tree 8, 4, 2, 1."""
    N = len(rowptr) - 1
    lanes = np.zeros((N, ROWSUM_GROUP))
    for i in range(N):
        for e in range(rowptr[i], rowptr[i + 1]):
            a = np.float64(val[e])
            lanes[i, (e - rowptr[i]) % ROWSUM_GROUP] += a * w[col[e]] if w is not None else a
    for s in (8, 4, 2, 1):
        lanes = lanes + lanes[:, np.arange(ROWSUM_GROUP) ^ s]
    return lanes[:, 0].copy()


def restated_cheb_step(rowptr, col, val, scale, X, prev, alpha, gamma, beta):
    """jamie_graph_cheb_step in numpy, rounding for rounding: acc = acc + (val[e] * scale[j]) * X[j, :] over the entries of a row
    in ascending order, then ((alpha * scale[i]) * acc + gamma * X[i, :]) - beta * prev[i, :]."""
    N, B = X.shape
    lens = np.diff(rowptr)
    acc = np.zeros((N, B))
    for p in range(int(lens.max()) if N else 0):
        rows = np.nonzero(lens > p)[0]
        e = rowptr[rows] + p
        j = np.asarray(col[e], np.int64)
        c = val[e].astype(np.float64) * scale[j]
        acc[rows] = acc[rows] + c[:, None] * X[j]
    out = (alpha * scale)[:, None] * acc + gamma * X
    if prev is not None:
        out = out - beta * prev
    return out


def cheb_reference(rowptr, col, val, scale, X, prev, alpha, gamma, beta):
    """(value, magnitude, row lengths): the step in extended precision (numpy longdouble, so that the reference's own rounding
    does not use up the bound) and the sum of the magnitudes of every element's terms."""
    ld = np.longdouble
    N, B = X.shape
    lens = np.diff(rowptr)
    row = np.repeat(np.arange(N), lens)
    j = np.asarray(col, np.int64)
    w = alpha * scale[row].astype(ld) * val.astype(ld) * scale[j].astype(ld)
    terms = w[:, None] * X[j].astype(ld)
    value, mag = np.zeros((N, B), ld), np.zeros((N, B), ld)
    np.add.at(value, row, terms)
    np.add.at(mag, row, np.abs(terms))
    own = ld(gamma) * X.astype(ld)
    value, mag = value + own, mag + np.abs(own)
    if prev is not None:
        last = ld(beta) * prev.astype(ld)
        value, mag = value - last, mag + np.abs(last)
    return value, mag, lens


def cheb_bound(lens):
    """Roundings an element's terms pass at most, in units of 2^-53 of the sum of their magnitudes: one owner
    sums the whole row (G = 1), so ceil(len / G) + log2 G + 8 = len + 8.  The chosen order needs len + 6: two products per term,
    len sums, alpha * scale, its product with the sum, and the two sums of the epilogue."""
    return (lens + 8)[:, None] * U


# ---- the restatement of the solver, block for block ----
def restated_eigen(S_apply, degree, k, tol=1e-8, max_iter=100, max_degree=60, seed=0):
    """`spectral.eigen` in float64 numpy: the same start, the same host-side functions of jamie_amd/spectral.py for the B x B
    problems and the filter's coefficients, numpy products where the device route launches a kernel.  S_apply(X) is S X."""
    from jamie_amd import spectral as jsp
    B = jsp.block_width(k)

    def orth(Y):
        for _ in range(2):
            Y = Y @ jsp.whitening(Y.T @ Y)
        return Y

    def rr(X):
        SX = S_apply(X)
        theta, V = jsp.ritz(X.T @ SX)
        X, SX = X @ V, SX @ V
        R = SX - X * theta[None, :]
        return theta, X, SX, np.sqrt(np.diag(R.T @ R))

    theta, X, SX, resid = rr(orth(jsp.start_block(degree, B, seed)))
    applies, iterations, degrees = 1, 0, []
    while not np.max(resid[:k]) <= tol and iterations < max_iter:
        p, e, c, sigma1 = jsp.filter_plan(theta, max_degree)
        prev, cur = None, X
        for al, ga, be in jsp.filter_coefficients(p, e, c, sigma1):
            nxt = al * S_apply(cur) + ga * cur - (be * prev if prev is not None else 0.0)
            prev, cur = cur, nxt
        applies += p
        degrees.append(p)
        iterations += 1
        theta, X, SX, resid = rr(orth(cur))
    return dict(vectors=X[:, :k].copy(), eigenvalues=theta[:k].copy(), residuals=resid[:k].copy(),
                converged=bool(np.max(resid[:k]) <= tol), iterations=iterations, applies=applies, degrees=degrees)


# ---- the derived checks of a solution ----
def gap_of(lam, k):
    return float(lam[k - 1] - lam[k])


def check_solution(Q, theta, S, lam, V, k, B, tol=None, same_graph=True, subspace_only=False, tag=''):
    """Checks (b) .. (f) of k returned eigenpairs (Q [N, k], theta [k]) against the reference eigh (lam descending, V) of the
    dense S; every figure is printed before it is asserted.  The residual R = S Q - Q Theta is taken on the reference's S: Kahan's
    and Davis-Kahan's bounds then hold for any orthonormal Q, whichever graph Q was computed on (`same_graph` False: the host
    route's graph differs from the device's in the last bit of some fp32 values, and check (b) against tol is left to the caller's
    own graph)."""
    N = len(Q)
    R = S @ Q - Q * theta[None, :]
    r = np.linalg.norm(R, axis=0)
    RF = float(np.linalg.norm(R))
    ortho = float(np.max(np.abs(Q.T @ Q - np.eye(k))))
    ortho_bound = 6.0 * (N * B + B * (B + 1)) * U
    gap = gap_of(lam, k)
    assert gap >= GAP, (tag, 'the precondition on the reference', gap)
    val_err = np.abs(theta - lam[:k])
    P = Q - V[:, :k] @ (V[:, :k].T @ Q)
    sub = float(np.linalg.norm(P, 2))
    sub_bound = RF / (gap - RF)
    print(f'{tag}: N = {N}, k = {k}, gap {gap:.2e}, residuals <= {r.max():.2e}, |R|_F {RF:.2e}, |Q^T Q - I| {ortho:.2e} (bound '
          f'{ortho_bound:.2e}), eigenvalue error {val_err.max():.2e}, subspace {sub:.2e} (bound {sub_bound:.2e})')
    if same_graph and tol is not None:
        assert np.all(r <= tol + 1e-12), (tag, r)                                     # (b)
    assert ortho <= ortho_bound, (tag, ortho)                                         # (c)
    assert sub <= sub_bound, (tag, sub, sub_bound)                                    # (e)
    if subspace_only:
        return dict(RF=RF, gap=gap, ortho=ortho, sub=sub, isolated=0)
    assert np.all(val_err <= RF), (tag, val_err, RF)                                  # (d)
    isolated = 0
    for i in range(k):                                                                # (f)
        below = lam[i] - lam[i + 1]
        above = lam[i - 1] - lam[i] if i else np.inf
        g = min(below, above)
        if g < GAP:
            continue
        isolated += 1
        cosine = abs(float(Q[:, i] @ V[:, i]))
        assert cosine >= 1.0 - (RF / g) ** 2 - N * U, (tag, i, cosine, RF, g)        # (N U: the dot product's own rounding)
        at = int(np.argmax(np.abs(Q[:, i])))
        assert Q[at, i] > 0, (tag, i, 'the sign rule')
    return dict(RF=RF, gap=gap, ortho=ortho, sub=sub, isolated=isolated)


def spearman(a, b):
    ra, rb = np.argsort(np.argsort(a)).astype(np.float64), np.argsort(np.argsort(b)).astype(np.float64)
    return float(np.corrcoef(ra, rb)[0, 1])

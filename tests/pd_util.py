"""Shared by tests/test_host_correspondence.py and tests/test_hip_prime_dual.py: the float64 reference of ONE Prime_Dual
iteration's element-wise work (jamie_pd_step, csrc/prime_dual.hip) from an arbitrary state, its staged pieces, a float32
restatement, the error bounds, the seeded state families and a guard-band allocator.  The reference half is plain numpy (no
torch); only `Arena` touches torch, and only when it is built.

The reference is written from jamie.py:357-394 as oracle.jamie_oracle.prime_dual states it, not from the kernel: column
vectors, the rank-one terms formed with vectors of ones, `1 - np.power(pho, i)` in double."""
import functools

import numpy as np

PHO1, PHO2, DELTA = 0.9, 0.999, 10e-8                                           # jamie.py:347-349
U = 2.0 ** -24                                                                  # unit roundoff of float32
STATE_KEYS = ('F', 'm1', 'm2', 'Mu', 'Lambda', 'S', 'rowsum', 'colsum')
VECTOR_ROWS = ('Mu', 'rowsum')                                                  # length m; Lambda, S, colsum have length n


# ---------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------
def pd_step_ref(state, G1, G2, alpha, iteration, rho, epsilon):
    """One iteration's element-wise work in float64.  G1 = (F Ky)(F^T (F Ky)) and G2 = Kx (F Ky) are the two products the
    gradient needs; `rowsum` = F 1 and `colsum` = F^T 1 are inputs of their own (the kernel reads them from the state).
    Returns (new state, T): T[r, c] is the sum of the magnitudes of the gradient's terms,
    4|G1| + 4|a||G2| + |Mu_r| + rho|rowsum_r| + |Lambda_c| + rho(|colsum_c| + |S_c| + 2)."""
    d = np.float64
    Fm, m1, m2 = (np.asarray(state[k], d) for k in ('F', 'm1', 'm2'))
    G1, G2, a = np.asarray(G1, d), np.asarray(G2, d), float(alpha)
    m, n = Fm.shape
    col = lambda k: np.asarray(state[k], d).reshape(-1, 1)   # noqa: E731
    Mu, Lambda, S, rowsum, colsum = col('Mu'), col('Lambda'), col('S'), col('rowsum'), col('colsum')
    Im, In = np.ones((m, 1)), np.ones((n, 1))
    grad = (4 * G1 - 4 * a * G2 + Mu @ In.T + Im @ Lambda.T                     # jamie.py:357-373
            + rho * (rowsum @ In.T + Im @ (colsum.T + (S - 2 * In).T)))
    i = int(iteration)
    m1 = PHO1 * m1 + (1 - PHO1) * grad                                          # jamie.py:375-381
    m2 = PHO2 * m2 + (1 - PHO2) * grad * grad
    step = (m1 / (1 - np.power(PHO1, i))) / (np.sqrt(m2 / (1 - np.power(PHO2, i))) + DELTA)
    F_tmp = Fm - step
    F_tmp[F_tmp < 0] = 0
    Fm = (1 - epsilon) * Fm + epsilon * F_tmp                                   # jamie.py:384
    grad_s = Lambda + rho * (Fm.T @ Im - In + S)                                # jamie.py:387-390
    s_tmp = S - grad_s
    s_tmp[s_tmp < 0] = 0
    S = (1 - epsilon) * S + epsilon * s_tmp
    Mu = Mu + epsilon * (Fm @ In - Im)                                          # jamie.py:393-394
    Lambda = Lambda + epsilon * (Fm.T @ Im - In + S)
    new = dict(F=Fm, m1=m1, m2=m2, Mu=Mu[:, 0], Lambda=Lambda[:, 0], S=S[:, 0], rowsum=(Fm @ In)[:, 0], colsum=(Fm.T @ Im)[:, 0],
               grad=grad)
    T = (4 * np.abs(G1) + 4 * abs(a) * np.abs(G2) + np.abs(col('Mu')) + rho * np.abs(rowsum)
         + np.abs(col('Lambda')).T + rho * (np.abs(colsum) + np.abs(col('S')) + 2).T)
    return new, T


def f_from_moments(F_old, m1_new, m2_new, iteration, epsilon, with_step=False):
    """The projected step and the epsilon-relaxation (jamie.py:378-384) in float64 from given moments."""
    F_old, m1, m2 = (np.asarray(x, np.float64) for x in (F_old, m1_new, m2_new))
    i = int(iteration)
    step = (m1 / (1 - np.power(PHO1, i))) / (np.sqrt(m2 / (1 - np.power(PHO2, i))) + DELTA)
    F = (1 - epsilon) * F_old + epsilon * np.maximum(F_old - step, 0)
    return (F, step) if with_step else F


def sums(F_new):
    F = np.asarray(F_new, np.float64)
    return F.sum(1), F.sum(0)


def duals(S, Mu, Lambda, rowsum_new, colsum_new, rho, epsilon):
    """The slack and dual updates (jamie.py:386-394) in float64 from given row / column sums.  Returns S, Mu, Lambda."""
    S, Mu, Lambda, rs, cs = (np.asarray(x, np.float64) for x in (S, Mu, Lambda, rowsum_new, colsum_new))
    grad_s = Lambda + rho * (cs - 1 + S)
    S_new = (1 - epsilon) * S + epsilon * np.maximum(S - grad_s, 0)
    return S_new, Mu + epsilon * (rs - 1), Lambda + epsilon * (cs - 1 + S_new)


def pd_step_staged(state, G1, G2, alpha, iteration, rho, epsilon):
    """The staged references composed (moments as pd_step_ref forms them): must equal pd_step_ref."""
    ref, _ = pd_step_ref(state, G1, G2, alpha, iteration, rho, epsilon)
    F = f_from_moments(state['F'], ref['m1'], ref['m2'], iteration, epsilon)
    rs, cs = sums(F)
    S, Mu, Lambda = duals(state['S'], state['Mu'], state['Lambda'], rs, cs, rho, epsilon)
    return dict(F=F, m1=ref['m1'], m2=ref['m2'], Mu=Mu, Lambda=Lambda, S=S, rowsum=rs, colsum=cs)


def pd_step_f32(state, G1, G2, alpha, iteration, rho, epsilon):
    """The same iteration in numpy float32 in a plain order, the constants as the float32 oracle holds them (python doubles
    0.9, 1 - 0.9, 0.999, 1 - 0.999 and the bias corrections, each rounded once).  Only m1 and m2 are used to fix bounds
    (F32_E_M1, F32_E_M2 below); the rest serves the exactness check of the dyadic states."""
    f = np.float32
    F, m1, m2, G1, G2 = (np.asarray(x, f) for x in (state['F'], state['m1'], state['m2'], G1, G2))
    Mu, Lambda, S, rowsum, colsum = (np.asarray(state[k], f) for k in ('Mu', 'Lambda', 'S', 'rowsum', 'colsum'))
    rho, eps, a4 = f(rho), f(epsilon), f(4) * f(alpha)
    rterm = (Mu + rho * rowsum)[:, None]
    cterm = ((colsum + S) - f(2))[None, :]
    grad = (((f(4) * G1 - a4 * G2) + rterm) + Lambda[None, :]) + rho * cterm
    m1 = f(PHO1) * m1 + f(1 - PHO1) * grad
    m2 = f(PHO2) * m2 + (f(1 - PHO2) * grad) * grad
    d1, d2 = f(1 - np.power(PHO1, int(iteration))), f(1 - np.power(PHO2, int(iteration)))
    step = (m1 / d1) / (np.sqrt(m2 / d2) + f(DELTA))
    F = (f(1) - eps) * F + eps * np.maximum(F - step, f(0))
    rs, cs = F.sum(1, dtype=f), F.sum(0, dtype=f)
    grad_s = Lambda + rho * ((cs - f(1)) + S)
    S_new = (f(1) - eps) * S + eps * np.maximum(S - grad_s, f(0))
    out = dict(F=F, m1=m1, m2=m2, Mu=Mu + eps * (rs - f(1)), Lambda=Lambda + eps * ((cs - f(1)) + S_new), S=S_new, rowsum=rs, colsum=cs)
    assert all(v.dtype == np.float32 for v in out.values())
    return out


def pd_iterate_ref(Kx, Ky, dx, dy, iters, rho, epsilon, delay, literal=True, history=None):
    """pd_step_ref iterated from the zero state with every product in float64 numpy: what
    orc.prime_dual(..., dtype=torch.float64) computes.  `literal`: the scaling factor from the reference's own three products
    and trace(Kx Kx) (jamie.py:397-402); otherwise from sum(G2 o F) / sum(Kx o Kx^T), which needs no [m, m] product.
    Returns the state after `iters` iterations with G1, G2 (the next iteration's) and alpha added."""
    Kx, Ky = np.asarray(Kx, np.float64), np.asarray(Ky, np.float64)
    m, n = Kx.shape[0], Ky.shape[0]
    N = max(m, n)
    Kx = (Kx / N).astype(np.float32).astype(np.float64)                         # jamie.py:330-334 (.float())
    Ky = (Ky / N).astype(np.float32).astype(np.float64)
    a = np.sqrt(dy / dx)
    st = zero_state(m, n, np.float64)
    trkk = np.trace(Kx @ Kx) if literal else float((Kx * Kx.T).sum())
    G1 = G2 = np.zeros((m, n))
    for i in range(1, iters + 1):
        FKy = st['F'] @ Ky
        G1, G2 = FKy @ (st['F'].T @ FKy), Kx @ FKy
        st, _ = pd_step_ref(st, G1, G2, a, i, rho, epsilon)
        if i >= delay:
            FKy = st['F'] @ Ky
            with np.errstate(invalid='ignore', divide='ignore'):
                a = (np.trace(Kx @ (FKy @ st['F'].T)) if literal else float(((Kx @ FKy) * st['F']).sum())) / trkk
        if history is not None:
            history.append(float(a))
    FKy = st['F'] @ Ky
    return dict(st, G1=FKy @ (st['F'].T @ FKy), G2=Kx @ FKy, alpha=a)


# ---------------------------------------------------------------------------------------------------
# Scaled errors and bounds
# ---------------------------------------------------------------------------------------------------
def moment_errors(m1, m2, ref, state, T):
    """(e_m1, e_m2): max |m1 - ref| / (0.9 |m1_old| + 0.1 T) and max |m2 - ref| / (0.999 m2_old + 0.001 T^2).  T >= 2 rho > 0."""
    m1o, m2o = np.asarray(state['m1'], np.float64), np.asarray(state['m2'], np.float64)
    e1 = np.abs(np.asarray(m1, np.float64) - ref['m1']) / (PHO1 * np.abs(m1o) + (1 - PHO1) * T)
    e2 = np.abs(np.asarray(m2, np.float64) - ref['m2']) / (PHO2 * m2o + (1 - PHO2) * T * T)
    assert np.isfinite(e1).all() and np.isfinite(e2).all(), 'non-finite scaled error'
    return float(e1.max()), float(e2.max())


# pd_step_f32 against pd_step_ref, maximum over measured_cases(): every state family, shape and iteration number of the GPU
# tests.  Measured on the CPU by tests/test_host_correspondence.py::test_fp32_restatement_fixes_the_moment_bounds, which asserts
# that the measurement lies in [0.9, 1.0] of each constant, so they cannot drift.  The GPU kernel is held to 4 x: hipcc may
# contract the updates into fma and associates the gradient's terms its own way (the same rule as optim_util.py).
F32_E_M1 = 2.4e-7    # measured 2.3682e-07 (adversarial, 5 x 1030, iteration 100000: the gradient's two large terms cancel)
F32_E_M2 = 4.1e-7    # measured 4.0777e-07 (the same case)
BOUND_M1, BOUND_M2 = 4 * F32_E_M1, 4 * F32_E_M2


def f_bound(F_old, step, epsilon):
    """|F_kernel - f_from_moments(kernel's moments)| elementwise.  With u = 2^-24 and the moments given exactly:
    step = (m1 / d1) / (sqrt(m2 / d2) + delta): d1, d2 rounded to float32 and the two divisions 2u each, halved by the root to
    u, the root u, the addition u, the last division u: 6u |step|.  t = f - step: u(|f| + |step|); max(., 0) is 1-Lipschitz, so
    the kink needs no exclusion.  eps as float32 and the product eps * t: 2u.  1 - eps: u, times f: u.  The final addition: u of
    the result.  Together 3u |f| + 10u eps (|f| + |step|); asserted with one more rounding on each part."""
    f, s = np.abs(np.asarray(F_old, np.float64)), np.abs(np.asarray(step, np.float64))
    return U * (4 * f + 12 * epsilon * (f + s))


def sum_bound(total, k):
    """A float32 sum of k non-negative terms in any order: every partial sum is at most the total, k - 1 additions."""
    return k * U * np.abs(np.asarray(total, np.float64))


def dual_bounds(S, Mu, Lambda, rs, cs, rho, epsilon):
    """(b_S, b_Mu, b_Lambda) against duals() of the same sums, u = 2^-24.  G = |Lambda| + rho(|cs| + 1 + |S|) bounds every
    intermediate of grad_s = Lambda + rho(cs - 1 + S): two additions, the product with rho and the last addition, 4u G.
    s_tmp = max(S - grad_s, 0): the subtraction u(|S| + G) <= 2u G, and max(., 0) is 1-Lipschitz, so the kink needs no
    exclusion: 6u G.  S' = (1 - eps) S + eps s_tmp: 1 - eps and its product 2u |S|; eps as float32 and its product 2u |s_tmp|
    <= 4u G on top of the 6u G; the last addition u(|S| + 2 eps G): 3u |S| + 12u eps G, asserted as 4u |S| + 14u eps G.
    Lambda' = Lambda + eps(cs - 1 + S'): H = |cs| + 1 + |S| + eps G >= |cs| + 1 + |S'|; two additions, eps and its product 4u H,
    the last addition u(|Lambda| + eps H), and S' carries b_S: u |Lambda| + 5u eps H + eps b_S, asserted as 2u |Lambda| + 6u eps
    H + eps b_S.  Mu' = Mu + eps(rs - 1) likewise: u |Mu| + 4u eps(|rs| + 1), asserted as 2u |Mu| + 4u eps(|rs| + 1).  Each lies
    below `4 roundings of G` (plain_dual_bounds; tests/test_host_correspondence.py asserts it)."""
    S, Mu, Lambda, rs, cs = (np.abs(np.asarray(x, np.float64)) for x in (S, Mu, Lambda, rs, cs))
    G = Lambda + rho * (cs + 1 + S)
    b_S = U * (4 * S + 14 * epsilon * G)
    H = cs + 1 + S + epsilon * G
    b_L = U * (2 * Lambda + 6 * epsilon * H) + epsilon * b_S
    b_Mu = U * (2 * Mu + 4 * epsilon * (rs + 1))
    return b_S, b_Mu, b_L


def plain_dual_bounds(S, Mu, Lambda, rs, cs, rho):
    """`A few (4) roundings of |Lambda| + rho(|cs| + 1 + |S|)`, and likewise for Mu: the ceiling dual_bounds stays under."""
    S, Mu, Lambda, rs, cs = (np.abs(np.asarray(x, np.float64)) for x in (S, Mu, Lambda, rs, cs))
    G = 4 * U * (Lambda + rho * (cs + 1 + S))
    return G, 4 * U * (Mu + rho * (rs + 1)), G


ALPHA_BLOCK = 256


def alpha_grid(count, n_partials):
    """The grid jamie_pd_alpha launches: one block per 1024 elements, at most n_partials, at least one."""
    return max(1, min(n_partials, (count // 4 + ALPHA_BLOCK - 1) // ALPHA_BLOCK))


def alpha_chain(count, n_partials):
    """Length of the longest chain of roundings between an input and alpha, from pd_dot_kernel / pd_alpha_kernel's order:
    the product and two levels of pairing inside a float4 (3), one addition per trip of the grid-stride loop, the tail term (1),
    the wave tree (4 lane exchanges + 2 levels over the rows) and the sum over the block's waves (<= 4): 10; in
    pd_alpha_kernel one addition per 256 partials, the same block sum (10) and the product with 1 / tr(Kx Kx) (1)."""
    grid = alpha_grid(count, n_partials)
    trips = -(-(count // 4) // (grid * ALPHA_BLOCK))
    return 3 + trips + 1 + 10 + -(-grid // ALPHA_BLOCK) + 10 + 1


def _block_sum_f32(v):
    """[blocks, 256] float32 -> [blocks]: a binary tree over each wave's 64 lanes, then the waves in turn."""
    w = v.reshape(v.shape[0], 4, 64)
    while w.shape[2] > 1:
        w = w[:, :, 0::2] + w[:, :, 1::2]
    t = np.zeros(v.shape[0], np.float32)
    for k in range(4):
        t = t + w[:, k, 0]
    return t


def alpha_f32(x, y, inv_trkk, n_partials):
    """sum(x o y) / tr(Kx Kx) in numpy float32 along a summation tree of the launch's shape (grid-stride trips, the tail in
    block 0, a tree per block, the partials): plain float32 arithmetic that alpha_bound must cover."""
    f = np.float32
    x, y = np.asarray(x, f).ravel(), np.asarray(y, f).ravel()
    count, grid = x.size, alpha_grid(x.size, n_partials)
    n4, span = count // 4, grid * ALPHA_BLOCK
    trips = -(-n4 // span)
    p = np.zeros((trips * span, 4), f)
    p[:n4] = (x[:4 * n4] * y[:4 * n4]).reshape(n4, 4)
    quad = ((p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])).reshape(trips, grid, ALPHA_BLOCK)
    acc = np.zeros((grid, ALPHA_BLOCK), f)
    for k in range(trips):
        acc = acc + quad[k]
    tail = count - 4 * n4
    acc[0, :tail] = acc[0, :tail] + x[4 * n4:] * y[4 * n4:]
    part = _block_sum_f32(acc)
    lanes = np.zeros(-(-grid // ALPHA_BLOCK) * ALPHA_BLOCK, f)
    lanes[:grid] = part
    s = np.zeros(ALPHA_BLOCK, f)
    for row in lanes.reshape(-1, ALPHA_BLOCK):
        s = s + row
    with np.errstate(invalid='ignore'):
        return _block_sum_f32(s[None, :])[0] * f(inv_trkk)


def alpha_bound(x, y, inv_trkk, n_partials):
    """|alpha_kernel - dot64(x, y) inv_trkk| <= gamma_k sum|x y| |inv_trkk| with k = alpha_chain (Higham's gamma_k = k u / (1 - k u))."""
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    k = alpha_chain(x.size, n_partials)
    return k * U / (1 - k * U) * float(np.abs(x * y).sum()) * abs(inv_trkk)


# ---------------------------------------------------------------------------------------------------
# State families (seeded; float32 arrays)
# ---------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (3, 2), (5, 3), (31, 255), (32, 256), (33, 257), (64, 512), (70, 260), (40, 252), (5, 1030), (100, 7),
          (97, 1024))
ITERATIONS = (1, 2, 10, 1000, 100000)
RHO = 10.0
EPSILONS = (1e-3, 1e-2)
DX, DY = 20, 14
DYADIC_EPSILON = 2.0 ** -6
DYADIC_SHAPES = ((40, 252), (33, 257))          # float4 path with a partly filled column tile; scalar path, two tiles each way


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def zero_state(m, n, dtype=np.float32):
    z = lambda *s: np.zeros(s, dtype)   # noqa: E731
    return dict(F=z(m, n), m1=z(m, n), m2=z(m, n), Mu=z(m), Lambda=z(n), S=z(n), rowsum=z(m), colsum=z(n))


def _case(name, state, G1, G2, alpha, iteration, rho, epsilon):
    f = np.float32
    return dict(name=name, state={k: np.ascontiguousarray(state[k], f) for k in STATE_KEYS}, G1=np.ascontiguousarray(G1, f),
                G2=np.ascontiguousarray(G2, f), alpha=f(alpha), iteration=int(iteration), rho=float(rho), epsilon=float(epsilon))


def zero(m, n, iteration=1, epsilon=1e-3):
    """The real start: everything 0 (so G1 = G2 = 0 too), alpha = sqrt(dy / dx)."""
    return _case('zero', zero_state(m, n), np.zeros((m, n)), np.zeros((m, n)), np.sqrt(DY / DX), iteration, RHO, epsilon)


def distances(m, n, seed=0):
    """Euclidean distance matrices Kx [m, m], Ky [n, n] of two noisy linear images of the same latent points."""
    r = _rng(11, m, n, seed)
    Z = r.standard_normal((max(m, n), 5))
    X, Y = Z[:m] @ r.standard_normal((5, DX)), Z[:n] @ r.standard_normal((5, DY))
    dist = lambda A: np.sqrt(np.maximum(((A[:, None, :] - A[None, :, :]) ** 2).sum(-1), 0))   # noqa: E731
    return dist(X), dist(Y)


@functools.lru_cache(maxsize=None)
def _warm_state(m, n, epsilon):
    Kx, Ky = distances(m, n)
    return pd_iterate_ref(Kx, Ky, DX, DY, 30, RHO, epsilon, 0, literal=False)


def warm(m, n, iteration, epsilon=1e-3):
    """What 30 iterations of the float64 reference reach (pd_iterate_ref, pinned to the oracle by the host tests), rounded to
    float32; rowsum and colsum are the sums of the rounded F.  `iteration` is the number the call is given."""
    w = _warm_state(m, n, epsilon)
    st = {k: np.asarray(w[k], np.float32) for k in STATE_KEYS}
    st['rowsum'], st['colsum'] = sums(st['F'])
    return _case('warm', st, w['G1'], w['G2'], w['alpha'], iteration, RHO, epsilon)


def adversarial(m, n, iteration, epsilon=1e-3, seed=0):
    """Signed Mu and Lambda; F >= 0 with a fifth exact zeros; moments of mixed sign with m2 >= 0 (a tenth exact zeros); G1 and
    G2 of magnitude ~5 with 4 G1 and 4 a G2 cancelling to ~1e-3 of it; S a third exact zeros, a third placed within a few ulp of
    the kink S - grad_s = 0 of the slack update (solved in float64 for the column sums this very step produces), a third |N|."""
    r = _rng(13, m, n, iteration, seed)
    f = np.float32
    F = (np.abs(r.standard_normal((m, n))) * (r.random((m, n)) > 0.2) / m).astype(f)
    alpha = f(0.8 + 0.1 * r.random())
    G2 = (5 * (0.5 + r.random((m, n)))).astype(f)
    G1 = (float(alpha) * G2.astype(np.float64) * (1 + 1e-3 * r.standard_normal((m, n)))).astype(f)
    m1 = (3 * r.standard_normal((m, n))).astype(f)
    m2 = ((3 * r.standard_normal((m, n))) ** 2 * (r.random((m, n)) > 0.1)).astype(f)
    rs, cs = sums(F)
    st = dict(F=F, m1=m1, m2=m2, Mu=r.standard_normal(m).astype(f), Lambda=r.standard_normal(n).astype(f),
              S=np.abs(r.standard_normal(n)).astype(f), rowsum=rs.astype(f), colsum=cs.astype(f))
    kind = r.integers(0, 3, n)
    st['S'][kind == 0] = 0
    ulps = r.integers(-3, 4, n)
    for _ in range(3):                  # S -> new column sums -> the S with S - grad_s = 0: a contraction (dF/dS ~ epsilon)
        new, _ = pd_step_ref(st, G1, G2, alpha, iteration, RHO, epsilon)
        kink = -(st['Lambda'].astype(np.float64) + RHO * (new['colsum'] - 1)) / (RHO - 1)
        st['S'] = np.where(kind == 1, kink, st['S']).astype(f)
    near = st['S'].copy()
    for k in range(1, 4):
        near = np.where(ulps >= k, np.nextafter(near, f(np.inf)), np.where(ulps <= -k, np.nextafter(near, f(-np.inf)), near))
    st['S'] = np.where(kind == 1, near, st['S']).astype(f)
    return _case('adversarial', st, G1, G2, alpha, iteration, RHO, epsilon)


def dyadic(m, n, seed=0):
    """Every input a small multiple of a power of two, rho = 10, epsilon = 2^-6, iteration 1, zero moments, and a gradient >= 4
    everywhere (4 G1 >= 8 against -4 a G2 >= -2, Mu + Lambda >= -2, rho(rowsum + colsum + S - 2) >= 0) over F <= 1/2.  Then
    the gradient, with every partial sum of it in any order, is exact in float32; the first step (m1 / d1) / (sqrt(m2 / d2) +
    delta) is 1 to a few ulp, so F - step < 0, F' = (1 - 2^-6) F exactly (multiples of 2^-9), and the row and column sums, the
    slack (both sides of its kink) and the duals are exact in any order too.  m1 = fl(fl(0.1) grad) and m2 = fl(fl(fl(0.001)
    grad) grad) are the same roundings however the compiler contracts them (the old moments are 0); they differ from the
    float64 reference only by the rounding of the two constants."""
    r = _rng(17, m, n, seed)
    q = lambda lo, hi, den, *s: (r.integers(lo, hi + 1, s) / den)   # noqa: E731
    st = zero_state(m, n)
    st['F'] = q(0, 4, 8, m, n)                                                  # multiples of 1/8 in [0, 1/2]
    st['rowsum'], st['colsum'] = q(8, 16, 8, m), q(8, 16, 8, n)                 # [1, 2]: inputs of their own
    st['Mu'], st['Lambda'] = q(-4, 4, 4, m), q(-4, 4, 4, n)
    st['S'] = q(0, 8, 4, n)
    st['F'][:, ::3] = 0                                                         # empty columns: S - grad_s > 0 there
    G1, G2 = q(16, 32, 8, m, n), q(0, 8, 8, m, n)
    return _case('dyadic', st, G1, G2, 0.5, 1, RHO, DYADIC_EPSILON)


def one_step_specs():
    """(family, m, n, iteration, epsilon) of the one-step GPU test: every shape and every iteration number with the adversarial
    state, both values of epsilon; the zero and the warm state on both paths and on the tile edges."""
    out = [('adversarial', m, n, ITERATIONS[k % len(ITERATIONS)], EPSILONS[k % 2]) for k, (m, n) in enumerate(SHAPES)]
    out += [('zero', 1, 1, 1, 1e-3), ('zero', 33, 257, 1, 1e-2), ('zero', 97, 1024, 1, 1e-3), ('zero', 70, 260, 1000, 1e-2)]
    out += [('warm', 3, 2, 2, 1e-3), ('warm', 33, 257, 10, 1e-2), ('warm', 64, 512, 1000, 1e-3), ('warm', 5, 1030, 100000, 1e-2),
            ('warm', 100, 7, 1, 1e-3), ('warm', 97, 1024, 10, 1e-2), ('warm', 32, 256, 100000, 1e-3)]
    return out


def spec_id(spec):
    family, m, n, it, eps = spec
    return f'{family}-{m}x{n}-i{it}-e{eps:g}'


def make_case(spec):
    family, m, n, it, eps = spec
    return {'zero': zero, 'warm': warm, 'adversarial': adversarial}[family](m, n, it, eps)


def one_step_cases():
    return [(spec_id(s), make_case(s)) for s in one_step_specs()]


def measured_cases():
    """Every (id, case) the float32 restatement is measured over: the one-step cases and the dyadic ones."""
    return one_step_cases() + [(f'dyadic-{m}x{n}', dyadic(m, n)) for m, n in DYADIC_SHAPES]


def run_ref(case):
    return pd_step_ref(case['state'], case['G1'], case['G2'], case['alpha'], case['iteration'], case['rho'], case['epsilon'])


def run_f32(case):
    return pd_step_f32(case['state'], case['G1'], case['G2'], case['alpha'], case['iteration'], case['rho'], case['epsilon'])


def check_one_step(case, got, say=print):
    """Every output of one jamie_pd_step call (`got`: name -> float32 numpy array, the eight state members after the call)
    against the references; prints each scaled error, then returns the list of failures (empty = pass)."""
    st, it, rho, eps = case['state'], case['iteration'], case['rho'], case['epsilon']
    m, n = st['F'].shape
    bad = []

    def judge(name, err, bound):
        err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
        ratio = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)))) if err.size else 0.0
        say(f'  {name}: max error / bound = {ratio:.3f}')
        if not ratio <= 1.0:
            bad.append(f'{name}: {ratio:.3f} of its bound')

    for k in STATE_KEYS:
        if not np.isfinite(got[k]).all():
            bad.append(f'{k}: non-finite values')
    if bad:
        return bad
    ref, T = run_ref(case)
    e1, e2 = moment_errors(got['m1'], got['m2'], ref, st, T)
    say(f'  e_m1 = {e1:.3e} (bound {BOUND_M1:.1e})   e_m2 = {e2:.3e} (bound {BOUND_M2:.1e})')
    if not e1 <= BOUND_M1:
        bad.append(f'm1: scaled error {e1:.3e} > {BOUND_M1:.1e}')
    if not e2 <= BOUND_M2:
        bad.append(f'm2: scaled error {e2:.3e} > {BOUND_M2:.1e}')
    F64, step = f_from_moments(st['F'], got['m1'], got['m2'], it, eps, with_step=True)
    judge('F given the moments', np.abs(got['F'] - F64), f_bound(st['F'], step, eps))
    if (got['F'] < 0).any():
        bad.append('F < 0')
    rs, cs = sums(got['F'])
    judge('rowsum', np.abs(got['rowsum'] - rs), sum_bound(rs, n))
    judge('colsum', np.abs(got['colsum'] - cs), sum_bound(cs, m))
    S, Mu, Lam = duals(st['S'], st['Mu'], st['Lambda'], got['rowsum'], got['colsum'], rho, eps)
    b_S, b_Mu, b_L = dual_bounds(st['S'], st['Mu'], st['Lambda'], got['rowsum'], got['colsum'], rho, eps)
    judge('S', np.abs(got['S'] - S), b_S)
    judge('Mu', np.abs(got['Mu'] - Mu), b_Mu)
    judge('Lambda', np.abs(got['Lambda'] - Lam), b_L)
    return bad


# ---------------------------------------------------------------------------------------------------
# Guard-band allocator (torch; device buffers for the GPU tests)
# ---------------------------------------------------------------------------------------------------
SENTINEL_BITS = 0x7FC5A5A5          # a quiet NaN with a payload: a read of a guard poisons the result, a write changes the bits
GUARD = 64                          # floats on either side of every buffer


class Arena:
    """Buffers carved out of one float32 tensor pre-filled with the sentinel.  `aligned` buffers start on a 16-byte boundary;
    the others start one float past one, so nothing can lean on an alignment the C ABI does not ask for.  Every buffer has
    GUARD sentinel floats on both sides; `violations()` names the buffers whose guards changed."""

    def __init__(self, sizes, aligned, device='cuda'):
        import torch
        self.torch = torch
        self.spans, off = {}, 0
        for name, size in sizes.items():
            off += GUARD
            off = (off + 3) // 4 * 4 + (0 if name in aligned else 1)
            self.spans[name] = (off, int(size))
            off += int(size)
        total = off + GUARD
        self.bits = torch.full((total,), SENTINEL_BITS, dtype=torch.int32, device=device)
        self.buf = self.bits.view(torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        self.t = {name: self.buf[o:o + s] for name, (o, s) in self.spans.items()}
        for name in aligned:
            assert self.t[name].data_ptr() % 16 == 0

    def violations(self):
        """Names of the buffers with a changed guard word before or after them."""
        edges = sorted((o, o + s, name) for name, (o, s) in self.spans.items())
        bad, prev_end = [], 0
        ok = (self.bits == SENTINEL_BITS).cpu().numpy()
        for k, (lo, hi, name) in enumerate(edges):
            nxt = edges[k + 1][0] if k + 1 < len(edges) else ok.size
            if not ok[prev_end:lo].all() or not ok[hi:min(nxt, hi + GUARD)].all():
                bad.append(name)
            prev_end = hi
        return bad

"""References of the device NMF evaluator (csrc/nmf.h; tests/test_nmf_host.py, tests/test_nmf_eval.py): a numpy RESTATEMENT of what
`sklearn.decomposition.NMF(solver='cd')` computes -

  * the solver: `_update_coordinate_descent` for all rows at once, `t` ascending (the rows of a factor do not depend on each other: only
    the coordinates inside a row are sequential), alternating W and H, with `_fit_coordinate_descent`'s stop rule;
  * NNDSVDa: `_initialize_nmf(init='nndsvda')` from a given truncated SVD (U, S, V) in the place of sklearn's randomized one;

in float64 (or any dtype asked for).  `reverse=True` runs every product's sum in the opposite order (the entries of a row of X, the rows
of the Gram matrix, the components of the gradient): the same mathematics, another rounding - the distance between the two is what any
fixed summation order may differ from sklearn by, and the bars of tests/test_nmf_eval.py are derived from it.

and the shared cases: the solver fixtures of tests/golden/nmf_eval.npz."""
import functools
import os

import numpy as np
from scipy.sparse import csr_matrix

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INIT_EPS = 1e-6     # `_initialize_nmf(eps=1e-6)`: NMF leaves it at its default

# name: (m, n, k, values given, empty row and column, component zeroed in the start, max_iter, tol)
SOLVER_CASES = {
    "70x45_values": (70, 45, 15, True, False, None, 50, 1e-4),
    "70x45_ones": (70, 45, 15, False, True, None, 50, 1e-4),
    "70x45_zero4": (70, 45, 15, False, False, 4, 50, 1e-4),
    "300x33_values": (300, 33, 16, True, False, None, 50, 1e-4),
    "300x33_ones": (300, 33, 16, False, False, None, 50, 1e-4),
    "33x129_values": (33, 129, 3, True, False, None, 50, 1e-4),
    "33x129_ones": (33, 129, 3, False, False, None, 50, 1e-4),
}
EARLY = "64x40_early"   # exact non-negative rank 3, k = 3, a start near the factors, tol = 1e-2: stops early
EARLY_TOL, EARLY_MAX_ITER = 1e-2, 50


def solver_inputs(name):
    """(X csr float64, W0 [m, k], H0 [k, n], max_iter, tol) of a solver case, rebuilt from its seed.  Stored values are multiples of 1/4
    (exact in float32, which is what the device's CSR holds)."""
    if name == EARLY:
        # the rows of B have disjoint supports, so H H^T is diagonal and one sweep over W lands on the factors: the violation falls from
        # v_1 to a few thousandths of it within the second iteration, clear of tol on both sides
        rng = np.random.RandomState(64)
        a = rng.randint(0, 4, size=(64, 3)).astype(np.float64)
        b = np.zeros((3, 40))
        b[rng.randint(0, 3, size=40), np.arange(40)] = rng.randint(1, 4, size=40)
        x = csr_matrix(a @ b)
        x.sort_indices()
        assert np.linalg.matrix_rank(x.toarray()) == 3
        w0 = a + 1.0 * rng.random_sample(a.shape)
        h0 = b + 0.004 * rng.random_sample(b.shape)
        return x, w0, h0, EARLY_MAX_ITER, EARLY_TOL
    m, n, k, values, empty, zeroed, max_iter, tol = SOLVER_CASES[name]
    rng = np.random.RandomState(1000 * m + n + (7 if values else 0) + (0 if zeroed is None else 13))
    dense = (rng.random_sample((m, n)) < 0.3).astype(np.float64)
    if values:
        dense *= rng.randint(1, 21, size=(m, n)) / 4.0
    if empty:
        dense[1, :] = 0.0
        dense[:, 2] = 0.0
    x = csr_matrix(dense)
    x.sort_indices()
    w0 = 0.1 + rng.random_sample((m, k))
    h0 = 0.1 + rng.random_sample((k, n))
    if zeroed is not None:
        w0[:, zeroed] = 0.0
        h0[zeroed, :] = 0.0
    return x, w0, h0, max_iter, tol


@functools.lru_cache(maxsize=1)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "nmf_eval.npz")))


def normwise(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - want) / np.linalg.norm(want))


# ------------------------------------------------------------------------------------------------ the solver
def _spmm(x, f, reverse):
    """X f with every row's sum in CSR order, or in the opposite order."""
    if not reverse:
        return np.asarray(x @ f)
    flipped = x[:, ::-1].tocsr()
    flipped.sort_indices()
    return np.asarray(flipped @ f[::-1])


def update_cd(x, w, ht, reverse=False):
    """`_update_coordinate_descent(X, W, Ht)` without regularisation or shuffle: W [rows, k] is updated in place, the violation returned."""
    k = ht.shape[1]
    hht = (ht[::-1].T @ ht[::-1]) if reverse else (ht.T @ ht)
    xht = _spmm(x, ht, reverse).astype(w.dtype, copy=False)
    order = range(k - 1, -1, -1) if reverse else range(k)
    violation = w.dtype.type(0)
    for t in range(k):
        grad = -xht[:, t].copy()
        for r in order:
            grad += hht[t, r] * w[:, r]
        pg = np.where(w[:, t] == 0, np.minimum(0, grad), grad)
        violation += np.abs(pg).sum()
        if hht[t, t] != 0:
            w[:, t] = np.maximum(w[:, t] - grad / hht[t, t], 0)
    return violation


def fit(x, w0, h0, max_iter=50, tol=1e-4, reverse=False, dtype=np.float64):
    """`_fit_coordinate_descent`: (W [m, k], H [k, n], n_iter, violations [n_iter])."""
    x = csr_matrix(x).astype(dtype)
    x.sort_indices()
    xt = x.T.tocsr()
    xt.sort_indices()
    w = np.array(w0, dtype=dtype, order="C")
    ht = np.array(np.asarray(h0).T, dtype=dtype, order="C")
    violations = []
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        v = update_cd(x, w, ht, reverse) + update_cd(xt, ht, w, reverse)
        violations.append(float(v))
        if violations[0] == 0 or v / violations[0] <= tol:
            break
    return w, ht.T.copy(), n_iter, np.asarray(violations)


# ------------------------------------------------------------------------------------------------ NNDSVDa
def nndsvda(x, u, s, v, eps=INIT_EPS):
    """`_initialize_nmf(X, k, init='nndsvda')` from the truncated SVD u [m, k], s [k], v [k, n]: (W0 [m, k], H0 [k, n])."""
    u, v, s = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64), np.asarray(s, dtype=np.float64)
    w, h = np.zeros_like(u), np.zeros_like(v)
    w[:, 0] = np.sqrt(s[0]) * np.abs(u[:, 0])
    h[0, :] = np.sqrt(s[0]) * np.abs(v[0, :])
    for j in range(1, len(s)):
        a, b = u[:, j], v[j, :]
        a_p, b_p = np.maximum(a, 0), np.maximum(b, 0)
        a_n, b_n = np.abs(np.minimum(a, 0)), np.abs(np.minimum(b, 0))
        a_p_nrm, b_p_nrm = np.sqrt(a_p @ a_p), np.sqrt(b_p @ b_p)
        a_n_nrm, b_n_nrm = np.sqrt(a_n @ a_n), np.sqrt(b_n @ b_n)
        m_p, m_n = a_p_nrm * b_p_nrm, a_n_nrm * b_n_nrm
        if m_p > m_n:                      # strict: the negative pair on a tie
            uu, vv, sigma = a_p / a_p_nrm, b_p / b_p_nrm, m_p
        else:
            uu, vv, sigma = a_n / a_n_nrm, b_n / b_n_nrm, m_n
        lbd = np.sqrt(s[j] * sigma)
        w[:, j] = lbd * uu
        h[j, :] = lbd * vv
    w[w < eps] = 0
    h[h < eps] = 0
    avg = x_mean(x)
    w[w == 0] = avg
    h[h == 0] = avg
    return w, h


def x_mean(x):
    x = csr_matrix(x)
    return float(x.data.astype(np.float64).sum() / (x.shape[0] * x.shape[1]))


def nndsvda_from_components(x, components, singular_values, through_float32=False):
    """NNDSVDa from the right factor alone, as the device has it: U = X V^T / sigma in float64 from the float32 `components` [k, n]
    (`through_float32`: U rounded to float32 and back - the bar of the device's init is derived from that distance)."""
    v = np.asarray(components, dtype=np.float64)
    s = np.asarray(singular_values, dtype=np.float64)
    u = np.asarray(csr_matrix(x).astype(np.float64) @ v.T) / s[None, :]
    if through_float32:
        u = u.astype(np.float32).astype(np.float64)
    return nndsvda(x, u, s, v)

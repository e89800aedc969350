"""References of the device truncated-SVD evaluator (csrc/svd_eval.h; tests/test_svd_eval*.py).

  * the float64 ORACLE: `np.linalg.svd` of the dense matrix, the exact rank-k reconstruction A Vk^T Vk, and the host metrics of
    sdrm_amd/metrics.py on it - what `TruncatedSVD(k, n_iter=100)` converges to (test_svd_eval.py ties the two together);
  * a numpy RESTATEMENT of the device scheme, stage by stage, in the device's number formats: float32 panels and products, the Gram
    matrix, the Cholesky factor and the sums of Y R^-1 in float64, the closing eigenproblem in float64 on the host.  Sums run in numpy's
    order, not the kernels': the restatement agrees with the device to rounding, not to the bit.

and the shared inputs: the planted-block matrices and the ML-100k fixture's stacked matrix."""
import functools
import os

import numpy as np
from scipy.sparse import csr_matrix, vstack

from sdrm_amd import metrics
from sdrm_amd.pipeline import K_LIST, csr_from_npz

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PANEL = 32
PIVOT_REL = 2.0 ** -40


class Breakdown(Exception):
    pass


# ------------------------------------------------------------------------------------------------ inputs
def planted(m, n, k, seed, fill=None, empty=False, value=1.0):
    """A binary [m, n] matrix with k planted blocks of users x items (density 0.8 inside a block, 0.08 outside): k singular values
    stand clear of the bulk.  `fill`: row 0 and column 0 entirely ones (longer than any gather chunk).  `empty`: row 1 and column 1
    without an entry.  `value`: what the stored entries hold."""
    rng = np.random.RandomState(seed)
    dense = rng.random_sample((m, n)) < 0.08
    ub, ib = rng.randint(0, k, size=m), rng.randint(0, k, size=n)
    dense |= (ub[:, None] == ib[None, :]) & (rng.random_sample((m, n)) < 0.8)
    if fill:
        dense[0, :] = True
        dense[:, 0] = True
    if empty:
        dense[1, :] = False
        dense[:, 1] = False
    a = csr_matrix(dense.astype(np.float64) * value)
    a.sort_indices()
    return a


# (m, n, k of the fit) of the planted shapes the issue names: n % 4 != 0 throughout, 33 x 37 barely above the panel, 300 x 259 ten row tiles
PLANTED = {"33x37": (33, 37, 3), "70x61": (70, 61, 5), "300x259": (300, 259, 20)}


@functools.lru_cache(maxsize=None)
def planted_case(name):
    m, n, k = PLANTED[name]
    return planted(m, n, k, seed=m, fill=name == "300x259", empty=name == "70x61"), k


@functools.lru_cache(maxsize=1)
def ml100k_inputs():
    """(train, valid, synthetic) of the ML-100k fixture: the synthetic part is the train matrix with its rows permuted."""
    z = np.load(os.path.join(GOLDEN, "ml100k.npz"))
    train, valid = csr_from_npz(z, "train_test"), csr_from_npz(z, "valid")
    train.eliminate_zeros()
    train.data[:] = 1.0
    synthetic = train[np.random.RandomState(7).permutation(train.shape[0])].tocsr()
    return train, valid, synthetic


@functools.lru_cache(maxsize=1)
def ml100k_stacked():
    """What compute_mf_results stacks for only_synthetic=True: (combined csr [synthetic | 80 % of each valid user], lo, held-out csr)."""
    train, valid, synthetic = ml100k_inputs()
    test_data, valid_data = metrics.split_train_test_proportion_from_csr_matrix(valid.copy(), batch_size=1000, random_seed=123)
    combined = vstack([synthetic, test_data]).tocsr()
    combined.sort_indices()
    return combined, synthetic.shape[0], valid_data


# ------------------------------------------------------------------------------------------------ the oracle
def oracle(a, k):
    """(reconstruction A Vk^T Vk [m, n] float64, singular values [k], Vk [k, n]) by the exact SVD."""
    dense = np.asarray(a.todense(), dtype=np.float64)
    _, s, vt = np.linalg.svd(dense, full_matrices=False)
    vk = vt[:k]
    return (dense @ vk.T) @ vk, s[:k].copy(), vk


@functools.lru_cache(maxsize=None)
def case(name):
    """(matrix, k, oracle(matrix, k)) of a planted shape or of "ml100k" (the stacked matrix, k = 20): computed once, shared, not to be written to."""
    a, k = (ml100k_stacked()[0], 20) if name == "ml100k" else planted_case(name)
    return a, k, oracle(a, k)


def normwise(got, want):
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - want) / np.linalg.norm(want))


def per_user_metrics(scores, seen, heldout):
    """(recall [6, U], ndcg [6, U]) float64 of dense scores [U, n] with the items of `seen` (csr [U, n]) masked, by the host metrics."""
    masked = metrics.mask_training_examples(seen, np.array(scores, dtype=np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        rec = np.stack([metrics.recall_at_k_batch(masked, heldout, k=k) for k in K_LIST])
        ndcg = np.stack([metrics.NDCG_binary_at_k_batch(masked, heldout, k=k) for k in K_LIST])
    return rec.astype(np.float64), ndcg.astype(np.float64)


def rounded_means(rec, ndcg):
    return (np.array([np.round(np.nanmean(r), 4) for r in rec]), np.array([np.round(np.nanmean(r), 4) for r in ndcg]))


# ------------------------------------------------------------------------------------------------ the restatement
def product(a32, q):
    """k_svd_spmm: float32 operands, float32 sums."""
    return np.asarray(a32 @ q.astype(np.float32), dtype=np.float32)


def orth_once(y):
    """k_svd_gram / k_svd_chol / k_svd_apply: the Gram matrix of the float32 panel in float64, G = L L^T, Y <- Y L^-T in float64, rounded."""
    y64 = y.astype(np.float64)
    g = y64.T @ y64
    big = g.diagonal().max()
    if not big > 0:
        raise Breakdown
    l = np.zeros_like(g)
    work = g.copy()
    for j in range(PANEL):                       # right-looking, as the kernel: the pivot test needs every pivot
        d = work[j, j]
        if not d > PIVOT_REL * big:
            raise Breakdown
        l[j, j] = np.sqrt(d)
        l[j + 1:, j] = work[j + 1:, j] / l[j, j]
        work[j + 1:, j + 1:] -= np.outer(l[j + 1:, j], l[j + 1:, j])
    rinv = np.linalg.inv(l).T
    return (y64 @ rinv).astype(np.float32)


def orth(y):
    return orth_once(orth_once(y))


def start_panel(n, seed):
    return np.random.RandomState(seed).standard_normal((n, PANEL)).astype(np.float32)


def close(z, k):
    """The host's closing problem: z [n, 32] = A^T Y = B^T; eigh(B B^T), the top k rotated and normalised."""
    z64 = z.astype(np.float64)
    lam, u = np.linalg.eigh(z64.T @ z64)
    top = np.argsort(-lam)[:k]
    v = (z64 @ u[:, top]).T
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(np.float32), np.sqrt(np.maximum(lam[top], 0.0))


def fit(a, k, n_iter, q0):
    """sdrm_svd_fit: (components [k, n] float32, singular values [k] float64)."""
    a32 = a.astype(np.float32).tocsr()
    at32 = a32.T.tocsr()
    q = np.asarray(q0, dtype=np.float32)
    for it in range(n_iter + 1):
        y = orth(product(a32, q))
        q = product(at32, y)
        if it < n_iter:
            q = orth(q)
    return close(q, k)


def scores(a_rows, components):
    """sdrm_svd_scores: float32 throughout."""
    t = np.asarray(a_rows.astype(np.float32) @ components.T.astype(np.float32), dtype=np.float32)
    return t @ components.astype(np.float32)

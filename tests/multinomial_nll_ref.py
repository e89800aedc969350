"""float64 restatement of the pre-stage's loss head, written from the formula:

    lse[r]  = log sum_i exp(o[r,i])                       (max-subtracted)
    loss    = -(1/b) sum_r sum_i x[r,i] (o[r,i] - lse[r])
    g[r,i]  = scale (exp(o[r,i] - lse[r]) s_r - x[r,i]) / b,   s_r = sum_i x[r,i]

and the inputs of the GPU cases of tests/test_multinomial_nll.py, made from a seed."""
import numpy as np
from scipy.sparse import csr_matrix

from vae_encode_ref import rel_l2, rel_max  # noqa: F401  (the tests take the error measures from here)

# (b, n_items, density, kind): kind "ratings" = values 1..5, "ones" = all ones (data = null on the device), "zeros" = integer
# ratings 0..5 with stored zeros, "shifted" = logits 30 N(0,1) + 60 (an unsubtracted exponential overflows)
CASES = [
    (37, 1009, 0.05, "ratings"),
    (5, 8582, 0.004, "ones"),
    (16, 3125, 0.05, "zeros"),
    (9, 515, 0.1, "shifted"),
    (1, 3, 0.0, "ratings"),
    (300, 63, 0.1, "ratings"),
]


def nll(logits, x, scale=1.0):
    """(loss, lse [b], grad [b, n_items]) in float64 for dense or scipy sparse x [b, n_items]."""
    o = np.asarray(logits, np.float64)
    x = np.asarray(x.toarray() if hasattr(x, "toarray") else x, np.float64)
    b = o.shape[0]
    top = o.max(axis=1, keepdims=True)
    lse = top + np.log(np.exp(o - top).sum(axis=1, keepdims=True))
    loss = -(x * (o - lse)).sum() / b
    grad = float(scale) * (np.exp(o - lse) * x.sum(axis=1, keepdims=True) - x) / b
    return loss, lse[:, 0], grad


def case_inputs(i):
    """(logits float32 [b, n_items], scipy CSR float32 [b, n_items]) of case i; row 0 is empty in every case (the (1, 3) case is
    that row alone), the column indices ascend within a row and no column appears twice."""
    b, n_items, density, kind = CASES[i]
    rng = np.random.RandomState(900 + i)
    logits = rng.standard_normal((b, n_items))
    logits = (30.0 * logits + 60.0 if kind == "shifted" else 2.0 * logits).astype(np.float32)
    indptr, indices, data = [0], [], []
    for r in range(b):
        if r > 0:
            cols = np.flatnonzero(rng.random_sample(n_items) < density)
            if cols.size == 0:
                cols = np.asarray([rng.randint(n_items)])
            indices.append(cols)
            if kind == "ones":
                data.append(np.ones(cols.size))
            else:
                data.append(rng.randint(0 if kind == "zeros" else 1, 6, size=cols.size))
        indptr.append(indptr[-1] + (indices[-1].size if r > 0 else 0))
    indices = np.concatenate(indices).astype(np.int32) if indices else np.zeros(0, np.int32)
    data = np.concatenate(data).astype(np.float32) if data else np.zeros(0, np.float32)
    return logits, csr_matrix((data, indices, np.asarray(indptr, np.int64)), shape=(b, n_items))


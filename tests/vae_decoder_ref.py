"""float64 restatement of the VAE decoder and the multinomial loss in train mode, written from the formulas:

    h3     = tanh(z W3^T + b3)                         [b, H]      W3 [H, L], b3 [H]
    logits = h3 W4^T + b4                              [b, I]      W4 [I, H], b4 [I]
    lse[r] = log sum_i exp(logits[r, i])               (max-subtracted)
    loss   = -(1/b) sum_r sum_p x_p (logits[r, col_p] - lse[r])
    g      = scale (exp(logits - lse) s_r - X) / b     s_r = sum_p x_p
    dW4 = g^T h3 ;  db4 = sum_r g[r, :] ;  dpre3 = (g W4)(1 - h3^2)
    dW3 = dpre3^T z ;  db3 = sum_r dpre3[r, :] ;  dz = dpre3 W3

and the inputs of the cases of tests/test_vae_decoder_train.py, made from seeds."""
import numpy as np
from scipy.sparse import csr_matrix

from sdrm_amd import synth
from vae_encode_ref import rel_l2, rel_max  # noqa: F401  (the tests take the error measures from here)

SCALE = 0.7
EXTRA_ROWS, ROW0 = 7, 3       # feed rows beyond the batch; first row of a contiguous batch

# (latent, hidden, n_items, b), each the smallest shape that reaches one thing a kernel can get wrong:
CASES = [
    (5, 37, 70, 33),          # no width on any grid; fewer columns than threads of a row's work-group; row stride off 16 bytes
    (40, 200, 1283, 300),     # ADM's widths; several row tiles; odd n_items above 1024: unrolled and tail loops, the 16-byte peel differs per row
    (83, 600, 1000, 130),     # odd latent; two row tiles plus two rows
    (830, 930, 1682, 65),     # ML-100k's widths; K of both GEMMs not a multiple of 32
    (16, 1030, 4099, 1),      # a single row; output K above 1024; n_items above 4096 and odd
    (4, 8, 40, 8200),         # batch above one weight-gradient K chunk: two slabs added in order
]


def special_rows(b):
    """(empty, full): the feed rows forced to hold no entry and every column; both inside ROW0 .. ROW0 + b - 1 when b allows."""
    return ROW0 + 1, (ROW0 + b - 2 if b >= 4 else ROW0)


def feed_of(n_rows, n_items, seed, ratings, empty, full):
    """`synth.synth_feed_csr` with row `empty` emptied and row `full` holding every column, forced into a feed of more than two rows.
    Canonical CSR, float32 values."""
    m = synth.synth_feed_csr(n_rows, n_items, 0.1, seed=seed, ratings=ratings)
    if n_rows <= 2:
        return m
    rng = np.random.RandomState(seed + 1)
    indptr, indices, data = [0], [], []
    for r in range(n_rows):
        if r == full:
            cols = np.arange(n_items, dtype=np.int32)
            vals = rng.randint(1, 6, size=n_items).astype(np.float32) if ratings else np.ones(n_items, np.float32)
        elif r == empty:
            cols, vals = np.zeros(0, np.int32), np.zeros(0, np.float32)
        else:
            cols, vals = m.indices[m.indptr[r]:m.indptr[r + 1]], m.data[m.indptr[r]:m.indptr[r + 1]]
        indices.append(cols)
        data.append(vals)
        indptr.append(indptr[-1] + len(cols))
    return csr_matrix((np.concatenate(data).astype(np.float32), np.concatenate(indices).astype(np.int32), np.asarray(indptr, np.int64)),
                      shape=(n_rows, n_items))


def forward(z, w3, b3, w4, b4, X, dtype=np.float64):
    """dict of h3, logits, lse and loss for the dense X [b, I]."""
    z, w3, b3, w4, b4, X = (np.asarray(t, dtype) for t in (z, w3, b3, w4, b4, X))
    h3 = np.tanh(z @ w3.T + b3)
    logits = h3 @ w4.T + b4
    mx = logits.max(axis=1, keepdims=True)
    lse = (mx + np.log(np.exp(logits - mx).sum(axis=1, keepdims=True)))[:, 0]
    loss = -np.sum(X * (logits - lse[:, None]), dtype=dtype) / dtype(z.shape[0])
    return dict(h3=h3, logits=logits, lse=lse, loss=loss)


def backward(fwd, z, w3, w4, X, scale=1.0, dtype=np.float64):
    """dict of g, dpre3, dz, dw3, db3, dw4, db4 from a `forward` result."""
    z, w3, w4, X = (np.asarray(t, dtype) for t in (z, w3, w4, X))
    h3, logits, lse = fwd["h3"], fwd["logits"], fwd["lse"]
    b = dtype(z.shape[0])
    g = dtype(scale) * (np.exp(logits - lse[:, None]) * X.sum(axis=1, keepdims=True) - X) / b
    dpre3 = (g @ w4) * (1 - h3 * h3)
    return dict(g=g, dpre3=dpre3, dz=dpre3 @ w3, dw3=dpre3.T @ z, db3=dpre3.sum(axis=0), dw4=g.T @ h3, db4=g.sum(axis=0))


def case_inputs(i):
    """dict of case i: z [b, L], w3 [H, L], b3 [H], w4 [I, H], b4 [I] float32; `m`, the feed [b + EXTRA_ROWS, I] (values 1..5 in
    cases 0, 1, 4, 5; all ones, i.e. no data array on the device, in cases 2, 3); the batch - `rows` [b] int64, distinct feed rows in a
    shuffled order (even cases) or None with `row0` = ROW0 (odd cases) - and its dense X [b, I]; scale; the widths."""
    latent, hidden, n_items, b = CASES[i]
    rng = np.random.RandomState(1300 + i)
    z = rng.standard_normal((b, latent)).astype(np.float32)
    w3 = (rng.standard_normal((hidden, latent)) / np.sqrt(latent)).astype(np.float32)
    b3 = (0.1 * rng.standard_normal(hidden)).astype(np.float32)
    w4 = (rng.standard_normal((n_items, hidden)) / np.sqrt(hidden)).astype(np.float32)
    b4 = (0.1 * rng.standard_normal(n_items)).astype(np.float32)
    ratings = (i // 2) % 2 == 0
    n_rows = b + EXTRA_ROWS
    empty, full = special_rows(b)
    m = feed_of(n_rows, n_items, 1400 + i, ratings, empty, full)
    if i % 2 == 0:
        if b == 1:
            rows = np.asarray([full], np.int64)
        else:                                           # the empty and the full row are in the batch
            others = np.setdiff1d(np.arange(n_rows), [empty, full])
            rows = rng.permutation(np.concatenate([[empty, full], rng.choice(others, size=b - 2, replace=False)])).astype(np.int64)
        row0, batch_rows = 0, rows
    else:
        rows, row0 = None, ROW0
        batch_rows = np.arange(ROW0, ROW0 + b)
    X = np.asarray(m[batch_rows].toarray(), np.float64)
    return dict(z=z, w3=w3, b3=b3, w4=w4, b4=b4, m=m, rows=rows, row0=row0, batch_rows=batch_rows, X=X, scale=SCALE, ratings=ratings,
                latent=latent, hidden=hidden, n_items=n_items, b=b)

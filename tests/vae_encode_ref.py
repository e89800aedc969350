"""numpy restatement of the frozen, eval-mode VAE encode hook (reference train_SDRM.py:241-250 with is_training == 0, dropout off):

    z  = mu = W2[:L] tanh(W1 x / max(|x|_2, 1e-12) + b1) + b2[:L]
    kl = -0.5 mean_rows sum(1 + logvar - mu^2 - exp(logvar)),   logvar = rows L..2L of the second Linear

`encode` in float64 (the yardstick of the GPU tests), `encode_csr_order32` in float32 with the first Linear summed entry by entry in
CSR order (what csrc/encode.h does, without its FMAs), and the inputs of the cases of tests/golden/vae_encode.npz, which the fixture
generator (tests/golden/make_vae_encode_golden.py) and the tests share."""
import os

import numpy as np
from scipy.sparse import csr_matrix

from sdrm_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# kind, n_items, hidden, latent, n, density, ratings, empty_row: the inputs of golden case i are made from this row alone
#   kind "ml100k": rows 0 .. n-1 of tests/golden/ml100k.npz `train_test` (real data: stored zeros, 18 .. 550 entries per row)
#   kind "synth":  synth.synth_feed_csr(n, n_items, density, seed=500 + i, ratings), row `empty_row` emptied when >= 0
# the encoder of case i is synth.synth_vae_encoder(n_items, hidden, latent, seed=400 + i)
CASES = [
    ("ml100k", 1008, 97, 30, 48, 0.0, 1, -1),
    ("synth", 3125, 120, 34, 33, 0.05, 1, -1),      # values 1..5 at about 5 % density
    ("synth", 257, 61, 17, 9, 0.08, 1, 3),          # an empty row
    ("synth", 101, 37, 5, 1, 0.1, 1, -1),           # n = 1
    ("synth", 1013, 203, 7, 21, 0.05, 1, -1),       # hidden and n_items not multiples of 4 (one wave per row)
    ("synth", 611, 601, 12, 19, 0.05, 1, 0),        # ... on the one-work-group-per-row kernel, first row empty
    ("synth", 203, 1030, 9, 11, 0.1, 1, -1),        # two float4 slices per thread
    ("synth", 97, 2050, 6, 7, 0.1, 0, -1),          # four
    ("synth", 64, 4100, 4, 5, 0.2, 1, -1),          # wider than the gather kernel's registers: densified
    ("synth", 8582, 200, 40, 24, 0.004, 0, -1),     # ADM-like: all ones, very sparse
]


def csr_from_npz(z, tag):
    shape = tuple(int(v) for v in z[tag + "_shape"])
    return csr_matrix((z[tag + "_data"].astype(np.float32), z[tag + "_indices"].astype(np.int32), z[tag + "_indptr"].astype(np.int64)), shape=shape)


def ml100k_train():
    return csr_from_npz(np.load(os.path.join(GOLDEN, "ml100k.npz")), "train_test")


def case_inputs(i):
    """(encoder tensors, scipy CSR float32 [n, n_items]) of golden case i."""
    kind, n_items, hidden, latent, n, density, ratings, empty_row = CASES[i]
    tensors = synth.synth_vae_encoder(n_items, hidden, latent, seed=400 + i)
    if kind == "ml100k":
        m = ml100k_train()[:n]
        assert m.shape[1] == n_items
    else:
        m = synth.synth_feed_csr(n, n_items, density, seed=500 + i, ratings=bool(ratings))
        if empty_row >= 0:
            keep = np.ones(n, bool)
            keep[empty_row] = False
            from scipy.sparse import diags
            m = (diags(keep.astype(np.float32)) @ m).tocsr()
            m.eliminate_zeros()
    m = csr_matrix((m.data.astype(np.float32), m.indices.astype(np.int32), m.indptr.astype(np.int64)), shape=m.shape)
    m.sort_indices()
    return tensors, m


def encode(x, w1, b1, w2, b2, dtype=np.float64):
    """(z [n, latent], kl) for a dense array or scipy sparse matrix x [n, n_items]."""
    x = np.asarray(x.toarray() if hasattr(x, "toarray") else x, dtype=dtype)
    w1, b1, w2, b2 = (np.asarray(t, dtype=dtype) for t in (w1, b1, w2, b2))
    norm = np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), dtype(1e-12))
    h = np.tanh((x / norm) @ w1.T + b1)
    out = h @ w2.T + b2
    L = w2.shape[0] // 2
    mu, logvar = out[:, :L], out[:, L:]
    kl = -0.5 * np.mean(np.sum(1 + logvar - mu * mu - np.exp(logvar), axis=1))
    return mu, kl


def encode_csr_order32(m, w1, b1, w2, b2):
    """The same in float32 with the first Linear as the sum, in CSR order, of the columns of W1 the row's entries name."""
    m = m.tocsr()
    w1t = np.ascontiguousarray(np.asarray(w1, np.float32).T)
    h = np.empty((m.shape[0], w1.shape[0]), np.float32)
    for r in range(m.shape[0]):
        acc, ss = np.zeros(w1.shape[0], np.float32), np.float32(0)
        for p in range(m.indptr[r], m.indptr[r + 1]):
            v = np.float32(m.data[p])
            acc = acc + v * w1t[m.indices[p]]
            ss = ss + v * v
        inv = np.float32(1) / max(np.sqrt(ss), np.float32(1e-12))
        h[r] = np.tanh(acc * inv + np.asarray(b1, np.float32))
    out = h @ np.asarray(w2, np.float32).T + np.asarray(b2, np.float32)
    L = w2.shape[0] // 2
    mu, logvar = out[:, :L], out[:, L:]
    kl = np.float32(-0.5) * np.mean(np.sum(1 + logvar - mu * mu - np.exp(logvar), axis=1, dtype=np.float32), dtype=np.float32)
    return mu, kl


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def rel_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))

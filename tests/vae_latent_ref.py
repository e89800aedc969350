"""float64 restatement of the VAE encoder behind its first pre-activation in train mode, written from the formulas:

    h1        = tanh(pre)                                              [b, H]
    out2      = h1 W2^T + b2 ;  mu = out2[:, :L], lv = out2[:, L:]     W2 [2L, H], b2 [2L]
    eps[r, j] = normal j & 3 of the column quad j >> 2 of feed row R_r: words = philox4x32_10(R_r, j >> 2, 9, step; key = seed),
                (n0, n1) = box_muller(x, y), (n2, n3) = box_muller(z, w)
    s         = exp(0.5 lv) ;  z = mu + eps s
    kl        = -0.5 / b sum_r sum_j (lv - mu^2 - expm1(lv))
    dmu       = gz + gkl mu / b ;  dlv = 0.5 gz eps s + 0.5 gkl expm1(lv) / b ;  dout2 = [dmu | dlv]
    dW2       = dout2^T h1 ;  db2 = sum_r dout2[r, :] ;  dpre = (dout2 W2) (1 - h1^2)

and the inputs of the cases of tests/test_vae_latent.py, made from seeds."""
import numpy as np

from oracle.philox_ref import _quad_normals, philox4x32_10
from vae_encode_ref import rel_l2, rel_max  # noqa: F401  (the tests take the error measures from here)

PURPOSE_VAE_EPS = 9
GKL = 0.2

# (hidden, latent, b), each for something a kernel can get wrong:
CASES = [
    (37, 5, 33),        # no width on any grid, a Philox quad cut by L, 2L below one tile
    (200, 40, 300),     # ADM's widths, several row tiles
    (600, 83, 130),     # odd L: the mu | logvar boundary inside a column tile and off 16 bytes; two row tiles plus two rows
    (930, 830, 65),     # ML-100k's widths, K not a multiple of 32
    (1030, 200, 1),     # a single row, K above 1024
]


def case_seed(i):
    return (0xD1B54A32D192ED03 + 1000003 * i) & (2 ** 63 - 1), 11 + i


def draw_eps(seed, step, row_ids, latent):
    """eps [len(row_ids), latent] float32 of the feed rows row_ids: a function of (seed, step, feed row, column) alone."""
    rows = np.asarray(row_ids, np.uint64)[:, None]
    quads = np.arange((latent + 3) // 4, dtype=np.uint64)[None, :]
    return _quad_normals(philox4x32_10(rows, quads, PURPOSE_VAE_EPS, step, seed), latent)


def forward(pre, w2, b2, eps, dtype=np.float64):
    """dict of h1, out2, mu, lv, z [.., float `dtype`] and kl."""
    pre, w2, b2, eps = (np.asarray(t, dtype) for t in (pre, w2, b2, eps))
    L = w2.shape[0] // 2
    h1 = np.tanh(pre)
    out2 = h1 @ w2.T + b2
    mu, lv = out2[:, :L], out2[:, L:]
    z = mu + eps * np.exp(dtype(0.5) * lv)
    kl = dtype(-0.5) / dtype(pre.shape[0]) * np.sum(lv - mu * mu - np.expm1(lv), dtype=dtype)
    return dict(h1=h1, out2=out2, mu=mu, lv=lv, z=z, kl=kl)


def backward(fwd, w2, eps, gz, gkl, dtype=np.float64):
    """dict of dout2, dpre, dw2, db2 from a `forward` result; gz or gkl None means zero."""
    w2, eps = np.asarray(w2, dtype), np.asarray(eps, dtype)
    mu, lv, h1 = fwd["mu"], fwd["lv"], fwd["h1"]
    b = dtype(mu.shape[0])
    gz = np.zeros_like(mu) if gz is None else np.asarray(gz, dtype)
    gkl = dtype(0.0 if gkl is None else gkl)
    dmu = gz + gkl * mu / b
    dlv = dtype(0.5) * gz * eps * np.exp(dtype(0.5) * lv) + dtype(0.5) * gkl * np.expm1(lv) / b
    dout2 = np.concatenate([dmu, dlv], axis=1)
    return dict(dout2=dout2, dpre=(dout2 @ w2) * (1 - h1 * h1), dw2=dout2.T @ h1, db2=dout2.sum(axis=0))


def case_inputs(i):
    """dict of case i: pre [b, H], w2 [2L, H], b2 [2L], gz [b, L], eps [b, L] (the injected noise) float32; gkl; rows [b] int64, the
    distinct feed rows of the batch, with row 0 and one above 2^16 among them (a batch of one row: the one above 2^16); seed, step."""
    hidden, latent, b = CASES[i]
    seed, step = case_seed(i)
    rng = np.random.RandomState(900 + i)
    pre = rng.standard_normal((b, hidden)).astype(np.float32)
    w2 = (rng.standard_normal((2 * latent, hidden)) / np.sqrt(hidden)).astype(np.float32)
    b2 = (0.1 * rng.standard_normal(2 * latent)).astype(np.float32)
    gz = (rng.standard_normal((b, latent)) / b).astype(np.float32)
    eps = rng.standard_normal((b, latent)).astype(np.float32)
    far = 2 ** 16 + 1 + int(rng.randint(1000))
    if b == 1:
        rows = np.asarray([far], np.int64)
    else:
        rows = rng.permutation(np.concatenate([[0, far], 1 + rng.choice(5000, size=b - 2, replace=False)])).astype(np.int64)
    return dict(pre=pre, w2=w2, b2=b2, gz=gz, eps=eps, gkl=GKL, rows=rows, seed=seed, step=step, hidden=hidden, latent=latent, b=b)

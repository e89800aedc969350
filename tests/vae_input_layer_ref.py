"""float64 restatement of the train-mode input layer of the VAE encoder, written from the formulas:

    keep(R, c) = word c & 3 of philox4x32_10(R, c >> 2, 7, step, seed) >= thr,   thr = floor(float64(float32(p)) 2^32)
    scale      = float32(1 / (1 - float64(float32(p))))
    rowscale_r = scale / max(sqrt(sum_c x[r,c]^2), 1e-12)                        (the norm covers dropped entries)
    x~[r,c]    = keep(R_r, c) rowscale_r x[r,c]                                  R_r the feed row of batch row r
    pre        = x~ W1^T + b1,    dW1 = dpre^T x~,    db1 = sum_r dpre[r,:]

and the inputs of the cases of tests/test_vae_input_layer.py, made from seeds."""
import numpy as np
from scipy.sparse import csr_matrix

from oracle.philox_ref import philox4x32_10
from vae_encode_ref import rel_l2, rel_max  # noqa: F401  (the tests take the error measures from here)

PURPOSE_VAE_DROP = 7
FEED_ROWS = 400
ALL_COLUMN = 3           # stored in every row of the feed but the empty row and the one-entry row
ROW_EMPTY, ROW_LONG, ROW_SINGLE = 0, 1, 2   # no entry / 600 entries (every usable column of a narrow feed) / one entry, dropped when p > 0
LO = 17                  # the batch's first place in the epoch's order

# (hidden, n_items, b, kind, p_drop): kind "ones" = all ones (data = null on the device), "zeros" = integer ratings 0..5 with stored
# zeros.  Batches of 33 hold the three special rows; the batch of 300 is rows that all store ALL_COLUMN; a batch of 1 is ROW_LONG.
CASES = [
    (37, 70, 33, "ones", 0.5),
    (200, 1009, 300, "zeros", 0.5),
    (600, 1009, 33, "ones", 0.3),
    (1030, 1009, 1, "zeros", 0.5),
    (1030, 70, 300, "ones", 0.0),
    (2052, 70, 33, "zeros", 0.5),    # above 2048: four slices per thread forward, a second pass over hidden in the weight gradient
]


def case_seed(i):
    return (0x9E3779B97F4A7C15 + 1000003 * i) & (2 ** 63 - 1), 3 + i


def threshold(p):
    return int(np.floor(np.float64(np.float32(p)) * 2.0 ** 32))


def scale(p):
    return np.float32(1.0 / (1.0 - np.float64(np.float32(p))))


def keep_bits(seed, step, rows, cols, p):
    """keep decision (bool) of the entries (rows[k], cols[k])."""
    rows, cols = np.broadcast_arrays(np.asarray(rows, np.uint64), np.asarray(cols, np.uint64))
    words = philox4x32_10(rows, cols >> np.uint64(2), PURPOSE_VAE_DROP, step, seed)
    sel = (cols & np.uint64(3)).astype(np.int64)
    word = np.choose(sel, list(words))
    return word >= np.uint64(threshold(p))


def keep_mask(seed, step, row_ids, n_items, p):
    """[len(row_ids), n_items] bool: the keep decision of every column of the feed rows row_ids."""
    row_ids = np.asarray(row_ids, np.int64)
    return keep_bits(seed, step, row_ids[:, None], np.arange(n_items)[None, :], p)


def forward(w1, b1, m, row_ids, seed, step, p):
    """(pre [b, hidden], rowscale [b], x~ [b, n_items]) in float64 for the rows row_ids of the scipy matrix m."""
    x = np.asarray(m[np.asarray(row_ids)].toarray(), np.float64)
    rowscale = np.float64(scale(p)) / np.maximum(np.sqrt((x * x).sum(axis=1)), 1e-12)
    xt = x * keep_mask(seed, step, row_ids, m.shape[1], p) * rowscale[:, None]
    return xt @ np.asarray(w1, np.float64).T + np.asarray(b1, np.float64), rowscale, xt


def backward(xt, dpre):
    """(dW1 [hidden, n_items], db1 [hidden]) in float64."""
    dpre = np.asarray(dpre, np.float64)
    return dpre.T @ xt, dpre.sum(axis=0)


def case_feed(n_items, kind, seed, step, p):
    """The 400-row feed of a case: canonical CSR, column n_items - 2 stored nowhere."""
    rng = np.random.RandomState(7000 + n_items + (1 if kind == "ones" else 0))
    usable = np.setdiff1d(np.arange(n_items), [n_items - 2])
    density = 0.05 if n_items > 256 else 0.12
    indptr, indices = [0], []
    single = None
    for c in usable[usable != ALL_COLUMN]:   # the one-entry row's column: the first one this case's draw drops (any, when p == 0)
        if p == 0 or not keep_bits(seed, step, [ROW_SINGLE], [c], p)[0]:
            single = int(c)
            break
    assert single is not None
    for r in range(FEED_ROWS):
        if r == ROW_EMPTY:
            cols = np.zeros(0, np.int64)
        elif r == ROW_LONG:
            others = usable[usable != ALL_COLUMN]
            cols = np.sort(np.append(rng.choice(others, size=min(600, usable.size) - 1, replace=False), ALL_COLUMN))
        elif r == ROW_SINGLE:
            cols = np.asarray([single])
        else:
            cols = np.union1d(usable[rng.random_sample(usable.size) < density], [ALL_COLUMN])
        indices.append(cols)
        indptr.append(indptr[-1] + cols.size)
    indices = np.concatenate(indices).astype(np.int32)
    data = np.ones(indices.size) if kind == "ones" else rng.randint(0, 6, size=indices.size)
    return csr_matrix((data.astype(np.float32), indices, np.asarray(indptr, np.int64)), shape=(FEED_ROWS, n_items))


def case_inputs(i):
    """dict of case i: w1 [hidden, n_items], b1 [hidden], dpre [b, hidden] float32; m the feed; order the epoch's order (a
    permutation of the 400 rows whose places LO .. LO + b - 1 are the batch); rows = order[LO:LO + b]; seed, step, p."""
    hidden, n_items, b, kind, p = CASES[i]
    seed, step = case_seed(i)
    rng = np.random.RandomState(800 + i)
    m = case_feed(n_items, kind, seed, step, p)
    if b == 1:
        batch = np.asarray([ROW_LONG])
    elif b == 33:
        batch = rng.permutation(np.concatenate([[ROW_EMPTY, ROW_LONG, ROW_SINGLE], 3 + rng.choice(FEED_ROWS - 3, size=b - 3, replace=False)]))
    else:
        batch = rng.permutation(np.concatenate([[ROW_LONG], 3 + rng.choice(FEED_ROWS - 3, size=b - 1, replace=False)]))
    rest = rng.permutation(np.setdiff1d(np.arange(FEED_ROWS), batch))
    order = np.concatenate([rest[:LO], batch, rest[LO:]]).astype(np.int64)
    w1 = (rng.standard_normal((hidden, n_items)) / np.sqrt(n_items)).astype(np.float32)
    b1 = (0.1 * rng.standard_normal(hidden)).astype(np.float32)
    dpre = rng.standard_normal((b, hidden)).astype(np.float32)
    return dict(w1=w1, b1=b1, dpre=dpre, m=m, order=order, rows=order[LO:LO + b].copy(), seed=seed, step=step, p=p, hidden=hidden,
                n_items=n_items, b=b, kind=kind)

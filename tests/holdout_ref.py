"""numpy restatement of the device hold-out split (sdrm_holdout_split, sdrm_amd/csrc/holdout.h), written from its definition:

    w_p     = word p & 3 of philox4x32_10(u, p >> 2, 8, draw, seed)          p the 0-based place of an entry inside feed row u
    rank(p) = #{q : w_q < w_p or (w_q == w_p and q < p)}                      = the place of p in a stable argsort of the words
    m_u     = 0 if n_u < 2 else min(n_u, math.ceil(test_prop * n_u))
    entry p is held out iff rank(p) < m_u; the others are the train part; both keep the CSR order of the columns

A row whose indptr pair is out of order or reaches outside [0, nnz], that is longer than n_items or holds a column outside
[0, n_items), and a row with fewer than two entries, is an empty row in both outputs.  Also the case feed of
tests/test_holdout_split.py, made from seeds."""
import math

import numpy as np
from scipy.sparse import csr_matrix

from oracle.philox_ref import philox4x32_10

PURPOSE_HOLDOUT = 8
HOLD_WAVE_MAX = 256      # csrc/holdout.h: the longest row a wave ranks
HOLD_TILE = 2048         # ... and the keys of one LDS tile of the work-group form
N_ITEMS = 4600
CASE_ROWS = 200
# every boundary of the wave form (4 entries per lane, 64 lanes, 256 per wave), of the work-group form's chunk (1024) and tile
BOUNDARY_LENGTHS = [0, 1, 2, 3, 4, 5, 6, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1025, HOLD_TILE + 1, N_ITEMS]


def held_count(test_prop, n):
    return 0 if n < 2 else min(int(n), math.ceil(test_prop * int(n)))


def words(seed, draw, u, n):
    """[..., n] uint64: the key words of the n entries of feed row u (`draw` may be an array [..., 1])."""
    p = np.arange(n, dtype=np.uint64)
    w = philox4x32_10(u, p >> np.uint64(2), PURPOSE_HOLDOUT, draw, seed)
    sel = np.broadcast_to((p & np.uint64(3)).astype(np.int64), w[0].shape)
    return np.choose(sel, list(w))


def held_mask(seed, draw, u, n, test_prop):
    """[..., n] bool: which entries of feed row u are held out."""
    w = words(seed, draw, u, n)
    order = np.argsort(w, axis=-1, kind="stable")
    mask = np.zeros(w.shape, dtype=bool)
    np.put_along_axis(mask, order[..., :held_count(test_prop, n)], True, axis=-1)
    return mask


def row_ok(indptr, indices, u, n_items, nnz):
    p0, p1 = int(indptr[u]), int(indptr[u + 1])
    if p0 < 0 or p1 < p0 or p1 > nnz or p1 - p0 > n_items:
        return False
    c = indices[p0:p1]
    return not ((c < 0) | (c >= n_items)).any()


def split(indptr, indices, n_items, test_prop, seed, draw):
    """(train_indptr, train_indices, held_indptr, held_indices) of the CSR arrays, int64 / int32, the index arrays of their filled
    length."""
    n_rows, nnz = len(indptr) - 1, len(indices)
    tr, he, tp, hp = [], [], [0], [0]
    for u in range(n_rows):
        n = int(indptr[u + 1] - indptr[u]) if row_ok(indptr, indices, u, n_items, nnz) else 0
        if n >= 2:
            cols = indices[int(indptr[u]):int(indptr[u]) + n]
            mask = held_mask(seed, draw, u, n, test_prop)
            tr.append(cols[~mask])
            he.append(cols[mask])
            tp.append(tp[-1] + int((~mask).sum()))
            hp.append(hp[-1] + int(mask.sum()))
        else:
            tp.append(tp[-1])
            hp.append(hp[-1])
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return np.asarray(tp, np.int64), cat(tr), np.asarray(hp, np.int64), cat(he)


def to_scipy(indptr, indices, n_items):
    indptr = np.asarray(indptr, np.int64)
    indices = np.asarray(indices[:int(indptr[-1])], np.int32)
    return csr_matrix((np.ones(indices.size, np.float32), indices, indptr), shape=(len(indptr) - 1, n_items))


def case_feed():
    """The case feed as a canonical scipy CSR matrix [CASE_ROWS, N_ITEMS] of integer ratings 1 .. 5: one row of every length of
    BOUNDARY_LENGTHS and rows of 8 .. 400 entries, in a shuffled order.  Returns (m, lengths)."""
    rng = np.random.RandomState(4600)
    lengths = np.asarray(BOUNDARY_LENGTHS + list(rng.randint(8, 401, size=CASE_ROWS - len(BOUNDARY_LENGTHS))))
    lengths = lengths[rng.permutation(CASE_ROWS)]
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(N_ITEMS, size=n, replace=False)) for n in lengths]).astype(np.int32)
    data = rng.randint(1, 6, size=indices.size).astype(np.float32)
    return csr_matrix((data, indices, indptr), shape=(CASE_ROWS, N_ITEMS)), lengths

"""References of the device CSR transpose and row stacking (csrc/csr_transpose.h; tests/test_csr_transpose.py).

  * the REFERENCE is scipy: `tocsr().tocsc()` + `sort_indices()` for the transpose, `scipy.sparse.vstack` for the stack.  Integers and
    float32 bit patterns: every comparison is `array_equal`, there is no tolerance.
  * a numpy RESTATEMENT of the device scheme - the row-blocked bit table W[B][c], the running popcounts off[B][c], the scan of the column
    counts and the place q = colptr[c] + off[B][c] + popc(W[B][c] & ((1 << j) - 1)) of entry (64 B + j, c) - with the kernels' checks: the
    index arithmetic can be debugged here without a device.

and the shared inputs: the smallest shapes that reach each boundary of the kernels."""
import functools

import numpy as np
from scipy.sparse import csr_matrix

import svd_eval_ref

BAD_PTR, BAD_COL, DUP = "indptr pair", "column index", "more than once"   # what sdrm_feed_status says for each of the transpose's bits


def popcount(w):
    w = np.ascontiguousarray(w, dtype=np.uint64)
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(w).astype(np.int64)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape + (8,)), axis=-1).sum(axis=-1).astype(np.int64)


# ------------------------------------------------------------------------------------------------ inputs
def _random(m, n, density, seed):
    a = csr_matrix((np.random.RandomState(seed).random_sample((m, n)) < density).astype(np.float64))
    a.sort_indices()
    return a


def _corners():
    """129 x 2050: three row blocks, columns behind one 2048-element scan chunk and behind a 64-column word; row 0 and column 0 entirely
    ones (the column is in every row block and longer than a wave), row 1 and column 1 empty, the last row and column occupied."""
    dense = np.random.RandomState(129).random_sample((129, 2050)) < 0.05
    dense[0, :] = True
    dense[:, 0] = True
    dense[1, :] = False
    dense[:, 1] = False
    dense[128, 2049] = True
    a = csr_matrix(dense.astype(np.float64))
    a.sort_indices()
    return a


CASES = ("1x1", "1x40", "40x1", "5x7-empty", "65x70", "129x2050", "70x61", "300x259", "ml100k", "700x4100")


@functools.lru_cache(maxsize=None)
def case(name):
    """The canonical all-ones scipy CSR matrix of a case: computed once, shared, not to be written to."""
    if name == "1x1":
        return csr_matrix(np.ones((1, 1)))
    if name == "1x40":
        return _random(1, 40, 0.5, 1)
    if name == "40x1":
        return _random(40, 1, 0.5, 2)
    if name == "5x7-empty":
        return csr_matrix((5, 7), dtype=np.float64)
    if name == "65x70":       # the second row block holds one row
        return _random(65, 70, 0.3, 65)
    if name == "129x2050":
        return _corners()
    if name in ("70x61", "300x259"):
        return svd_eval_ref.planted_case(name)[0]
    if name == "ml100k":      # 938 x 1008
        return svd_eval_ref.ml100k_stacked()[0]
    if name == "700x4100":
        return _random(700, 4100, 0.05, 700)
    raise KeyError(name)


def arrays(a, with_data, seed=0):
    """(indptr int64, indices int32, data float32 | None) of a canonical matrix; the values are distinct, so a misplaced one shows."""
    a = a.tocsr()
    data = (np.random.RandomState(seed).permutation(a.nnz) + 0.5).astype(np.float32) if with_data else None
    return a.indptr.astype(np.int64), a.indices.astype(np.int32), data


def shuffled(indptr, indices, data, seed=5):
    """The same matrix with the entries of every row in a random order, values along with them."""
    rng = np.random.RandomState(seed)
    order = np.concatenate([indptr[r] + rng.permutation(int(indptr[r + 1] - indptr[r])) for r in range(len(indptr) - 1)] + [np.zeros(0, np.int64)])
    order = order.astype(np.int64)
    return indptr, indices[order], None if data is None else data[order]


def scipy_transpose(indptr, indices, data, shape):
    """(colptr int64, rowidx int32, cdata float32 | None) by scipy; indptr may hold absolute offsets."""
    indptr = np.asarray(indptr, dtype=np.int64)
    lo, hi = int(indptr[0]), int(indptr[-1])
    vals = np.arange(1, hi - lo + 1, dtype=np.float64)   # the entry's place + 1: the values follow by a gather, whatever they are
    c = csr_matrix((vals, indices[lo:hi], indptr - lo), shape=shape).tocsc()
    c.sort_indices()
    place = c.data.astype(np.int64) - 1 + lo
    return c.indptr.astype(np.int64), c.indices.astype(np.int32), None if data is None else data[place]


# ------------------------------------------------------------------------------------------------ the restatement
def transpose_restated(indptr, indices, data, m, n, capacity=None):
    """sdrm_csr_transpose in numpy: (colptr [n + 1] int64, rowidx [capacity] int32, cdata [capacity] float32 | None, set of raised
    messages).  Places nothing was stored to hold -1 / nan."""
    capacity = len(indices) if capacity is None else capacity
    blocks = (m + 63) // 64
    table = np.zeros((blocks, n), dtype=np.uint64)
    raised, checked, rows = set(), 0, []
    for r in range(m):                                             # k_csrt_mark
        p0, p1 = int(indptr[r]), int(indptr[r + 1])
        if p0 < 0 or p1 < p0 or p1 > capacity:
            raised.add(BAD_PTR)
            continue
        c = indices[p0:p1].astype(np.int64)
        ok = (c >= 0) & (c < n)
        if not ok.all():
            raised.add(BAD_COL)
        p, c = np.arange(p0, p1)[ok], c[ok]
        np.bitwise_or.at(table[r >> 6], c, np.uint64(1) << np.uint64(r & 63))
        checked += len(c)
        rows.append((r, p, c))
    pop = popcount(table)                                          # k_csrt_colscan
    off = np.cumsum(pop, axis=0) - pop
    colptr = np.concatenate([[0], np.cumsum(pop.sum(axis=0))]).astype(np.int64)   # k_csr_scan
    if colptr[-1] != checked:                                      # k_csrt_fill
        raised.add(DUP)
    if colptr[-1] > capacity:
        raised.add(BAD_PTR)
    rowidx = np.full(capacity, -1, dtype=np.int32)
    cdata = None if data is None else np.full(capacity, np.nan, dtype=np.float32)
    for r, p, c in rows:
        below = (np.uint64(1) << np.uint64(r & 63)) - np.uint64(1)
        q = colptr[c] + off[r >> 6, c] + popcount(table[r >> 6, c] & below)
        keep = q < capacity
        rowidx[q[keep]] = r
        if data is not None:
            cdata[q[keep]] = data[p[keep]]
    return colptr, rowidx, cdata, raised

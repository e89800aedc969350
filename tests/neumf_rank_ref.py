"""numpy restatement of sdrm_neumf_rank_problem, sdrm_neumf_rank_users and the NeuMF footing of sdrm_rank_metrics_rows, written from the
text in include/sdrm_hip.h.  A part is (indptr int64 [n_rows + 1], indices int32 [capacity], n_rows, user0, label), indptr holding
absolute offsets into indices - tests/neumf_triples_ref.py's form."""
import numpy as np

BAD_ROW, BAD_COL, STACK_PTR = 1, 2, 64   # the feed status word's bits (csrc/csr_batch.h: FEED_BAD_ROW, FEED_BAD_COL, FEED_STACK_PTR)
ROW_TEXT, COL_TEXT, PTR_TEXT = "a row id outside", "a column index outside [0, n_items)", "sdrm_csr_vstack: an indptr pair"


def _csr(sets, n_rows):
    """(indptr int64 [n_rows + 1], indices int32) of per-row sets of columns: ascending, duplicate-free."""
    lengths = np.array([len(sets.get(u, ())) for u in range(n_rows)], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.array([c for u in range(n_rows) for c in sorted(sets.get(u, ()))], dtype=np.int32)
    return indptr, indices


def rank_problem_ref(parts, n_items, item_present, heldout, n_rows):
    """(cols int32 [C], (seen indptr, seen indices), (relevant indptr, relevant indices), counts (C, seen nnz, relevant nnz, dropped),
    status bits).  Rows are dense by user id: row u is user u."""
    item_present = np.asarray(item_present)
    cols = np.flatnonzero(item_present != 0).astype(np.int32)
    col_of = np.full(n_items, -1, dtype=np.int64)
    col_of[cols] = np.arange(cols.shape[0])
    status, seen = 0, {}
    for indptr, indices, rows_p, user0, _label in parts:
        indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32)
        capacity = indices.shape[0]
        for r in range(rows_p):
            p0, p1 = int(indptr[r]), int(indptr[r + 1])
            if p0 < 0 or p1 < p0 or p1 > capacity or p1 - p0 > n_items:
                status |= STACK_PTR
                continue
            row = indices[p0:p1]
            if np.any((row < 0) | (row >= n_items)):
                status |= BAD_COL
                continue
            if row.shape[0] == 0:
                continue
            if user0 + r >= n_rows:
                status |= BAD_ROW
                continue
            seen.setdefault(user0 + r, set()).update(int(col_of[c]) for c in row if col_of[c] >= 0)
    relevant, dropped = {}, 0
    for user, item, label in np.asarray(heldout, dtype=np.int64).reshape(-1, 3):
        defect = (BAD_ROW if user < 0 or user >= n_rows else 0) | (BAD_COL if item < 0 or item >= n_items else 0)
        if defect:
            status |= defect
            dropped += 1
        elif label > 0 and col_of[item] >= 0:
            relevant.setdefault(int(user), set()).add(int(col_of[item]))
    seen_csr, rel_csr = _csr(seen, n_rows), _csr(relevant, n_rows)
    return cols, seen_csr, rel_csr, (int(cols.shape[0]), int(seen_csr[1].shape[0]), int(rel_csr[1].shape[0]), dropped), status


def rank_users_ref(mask):
    return np.flatnonzero(np.asarray(mask) != 0).astype(np.int32)


def host_form(csr, n_cols=None):
    """(ids, indptr, indices) as sdrm_amd/neumf.py's RankingProblem keeps a matrix: the rows that hold an entry, by ascending id."""
    indptr, indices = csr
    lengths = np.diff(indptr)
    ids = np.flatnonzero(lengths).astype(np.int64)
    return ids, np.concatenate([[0], np.cumsum(lengths[ids])]).astype(np.int64), indices.astype(np.int32)


def select(csr, users, n_cols):
    """scipy CSR [len(users), n_cols] of the rows `users` of a dense-by-id matrix; an id outside it is an empty row."""
    from scipy.sparse import csr_matrix
    indptr, indices = csr
    n_rows = indptr.shape[0] - 1
    rows = [indices[indptr[u]:indptr[u + 1]] if 0 <= u < n_rows else indices[:0] for u in users]
    out_ptr = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int64)
    flat = np.concatenate(rows) if rows else indices[:0]
    return csr_matrix((np.ones(flat.shape[0], dtype=np.float32), flat, out_ptr), shape=(len(users), n_cols))


def neumf_footing(ndcg, n_true, idcg, n_cols, ks):
    """`rank_all_items`' host footing of `rank_metrics`' NDCG [nk, U]: three float64 operations, in this order."""
    out = np.array(ndcg, dtype=np.float64)
    for q, k in enumerate(ks):
        out[q] = np.where(n_true > 0, out[q] * idcg[np.minimum(n_true, k)] / idcg[min(n_cols, k)], 0.0)
    return out

"""numpy restatement of sdrm_neumf_triples, written from the text in include/sdrm_hip.h: the order, the row checks, the counts,
item_present and the status bits.  A part is (indptr int64 [n_rows + 1], indices int32 [capacity], n_rows, user0, label); indptr holds
absolute offsets into indices."""
import numpy as np

STACK_PTR, BAD_COL = 64, 2   # the feed status word's bits (csrc/csr_batch.h: FEED_STACK_PTR, FEED_BAD_COL)
PTR_TEXT, COL_TEXT = "sdrm_csr_vstack: an indptr pair", "a column index outside [0, n_items)"


def triples_ref(parts, n_items, capacity_out, before=None, with_present=True):
    """(out int32 [capacity_out, 3], counts (m, ones, max user + 1, max item + 1), item_present uint8 [n_items] | None, status bits):
    `out` starts as `before` (default: zeros) and only its rows 0 .. m - 1 are written."""
    out = np.zeros((capacity_out, 3), dtype=np.int32) if before is None else np.array(before, dtype=np.int32).reshape(capacity_out, 3)
    present = np.zeros(n_items, dtype=np.uint8) if with_present else None
    rows, status = [], 0
    for indptr, indices, n_rows, user0, label in parts:
        indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32)
        capacity = indices.shape[0]
        for r in range(n_rows):
            p0, p1 = int(indptr[r]), int(indptr[r + 1])
            if p0 < 0 or p1 < p0 or p1 > capacity or p1 - p0 > n_items:
                status |= STACK_PTR
                continue
            cols = indices[p0:p1]
            if np.any((cols < 0) | (cols >= n_items)):
                status |= BAD_COL
                continue
            rows.append(np.stack([np.full(cols.shape[0], user0 + r, dtype=np.int64), cols.astype(np.int64),
                                  np.full(cols.shape[0], label, dtype=np.int64)], axis=1))
    t = np.concatenate(rows) if rows else np.zeros((0, 3), dtype=np.int64)
    if t.shape[0] > capacity_out:   # rows that share entries: the triples behind capacity_out are dropped
        status |= STACK_PTR
        t = t[:capacity_out]
    m = t.shape[0]
    out[:m] = t.astype(np.int32)
    if with_present:
        present[t[:, 1]] = 1
    counts = (m, int((t[:, 2] == 1).sum()), int(t[:, 0].max()) + 1 if m else 0, int(t[:, 1].max()) + 1 if m else 0)
    return out, counts, present, status

"""numpy restatement of the NeuMF evaluator's epoch draw (sdrm_neumf_epoch_draw, sdrm_amd/csrc/neumf_draw.h), written from its
definition in include/sdrm_hip.h - TEST INFRASTRUCTURE.  Both functions are vectorised and both assert the walk bound.

perm(n, seed, epoch, draw): the keyed permutation of 0 .. n-1 - a balanced Feistel network over [0, 4^h) with six rounds keyed by word 0
of Philox4x32-10 at counter (R, r, 12 | draw << 8, epoch), and cycle walking back into [0, n).
epoch_draw(T, n_hold, seed, epoch, n_users): (hold, out, (n_pos, n_neg, m), present) as the device call leaves them."""
from __future__ import annotations

import numpy as np

from oracle import philox_ref as ph

PURPOSE_NEUMF_EPOCH = 12
MAX_WALKS = 1024
ROUNDS = 6


def half_bits(n):
    b = max(1, int(n - 1).bit_length())
    return (b + 1) // 2


def _feistel(x, h, seed, epoch, draw):
    mask = np.uint64((1 << h) - 1)
    L, R = x >> np.uint64(h), x & mask
    for r in range(ROUNDS):
        w = ph.philox4x32_10(R, r, PURPOSE_NEUMF_EPOCH | (draw << 8), epoch, seed)[0]
        L, R = R, L ^ (w & mask)
    return (L << np.uint64(h)) | R


def perm(n, seed=0, epoch=0, draw=0, walks_out=None):
    """int64 [n]: perm(i) for i = 0 .. n-1.  `walks_out`: a list that receives the longest walk."""
    n = int(n)
    assert n >= 1
    h = half_bits(n)
    x = np.arange(n, dtype=np.uint64)
    todo = np.arange(n)
    walks = 0
    while todo.size:
        walks += 1
        assert walks <= MAX_WALKS, f"perm({n}): a value walked {MAX_WALKS} times without coming back inside"
        x[todo] = _feistel(x[todo], h, seed, epoch, draw)
        todo = todo[x[todo] >= np.uint64(n)]
    if walks_out is not None:
        walks_out.append(walks)
    return x.astype(np.int64)


def epoch_draw(T, n_hold, seed=0, epoch=0, n_users=None):
    T = np.asarray(T)
    n = T.shape[0]
    assert T.ndim == 2 and T.shape[1] == 3 and 1 <= n_hold < n
    p0 = perm(n, seed, epoch, 0)
    hold, part = T[p0[:n_hold]], T[p0[n_hold:]]
    n_part = n - n_hold
    g = np.flatnonzero(part[:, 2] == 0)
    n_neg, n_pos = int(g.size), int((part[:, 2] == 1).sum())
    n_extra = n_pos if n_neg > 0 else 0
    if n_extra:
        k = np.arange(n_extra, dtype=np.uint64)
        words = np.stack(ph.philox4x32_10(k >> np.uint64(2), 0, PURPOSE_NEUMF_EPOCH | (1 << 8), epoch, seed))   # [4, n_extra]
        w = words[(k & np.uint64(3)).astype(np.int64), np.arange(n_extra)]
        both = np.concatenate([part, part[g[ph.bounded(w, n_neg)]]])
    else:
        both = part
    m = n_part + n_extra
    out = both[perm(m, seed, epoch, 2)]
    present = None
    if n_users is not None:
        present = np.zeros(n_users, dtype=np.uint8)
        u = hold[:, 0]
        present[u[(u >= 0) & (u < n_users)]] = 1
    return hold, out, (n_pos, n_neg, m), present

"""TEST INFRASTRUCTURE ONLY: float64 restatement of the evaluation half of a VAE pre-stage epoch (train_SDRM.py:160-177 with
is_training == 0 and dropout off), what sdrm_vae_eval_holdout (csrc/eval_half.h) computes.  For user u, with T_u the columns of the
train part and H_u those of the held part, every stored entry counting as 1:

    x = 1_{T_u} / max(sqrt(|T_u|), 1e-12);  h1 = tanh(W1 x + b1);  z = W2[:L] h1 + b2[:L];  h3 = tanh(W3 z + b3);  s = W4 h3 + b4
    score_u = Recall@k or NDCG@k of s against H_u with the items of T_u at -inf

The ranking is oracle/rank_metrics_ref.py's formulation - rank = #{better} + #{equal, lower index}, numpy's pairwise sum of the
discounts - kept in the dtype of the scores it is given (that module rounds its scores to float32 first).  Plain numpy: small cases."""
import numpy as np

from oracle.rank_metrics_ref import np_pairwise_sum


def weights_of(vae):
    """(w1, b1, w2, b2, w3, b3, w4, b4) float64 numpy arrays of a `VAE`, as `nn.Linear` stores them."""
    mods = (vae.encoder[0], vae.encoder[2], vae.decoder[0], vae.decoder[2])
    return tuple(t.detach().double().cpu().numpy() for m in mods for t in (m.weight, m.bias))


def logits(weights, train, dtype=np.float64):
    """s [n_rows, n_items] for the rows of the scipy CSR `train`, every operation in `dtype`."""
    w1, b1, w2, b2, w3, b3, w4, b4 = (np.asarray(t, dtype=dtype) for t in weights)
    L = w3.shape[1]
    train = train.tocsr()
    x = np.zeros(train.shape, dtype=dtype)
    for u in range(train.shape[0]):
        x[u, train.indices[train.indptr[u]:train.indptr[u + 1]]] = 1
    norm = np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), dtype(1e-12))
    h1 = np.tanh((x / norm) @ w1.T + b1)
    z = h1 @ w2[:L].T + b2[:L]
    h3 = np.tanh(z @ w3.T + b3)
    return h3 @ w4.T + b4


def masked(scores, train):
    out = np.array(scores, copy=True)
    train = train.tocsr()
    for u in range(out.shape[0]):
        out[u, train.indices[train.indptr[u]:train.indptr[u + 1]]] = -np.inf
    return out


def metrics(scores, train, held, k):
    """(recall [U], ndcg [U]) float64 at cut-off k of `scores` (any float dtype, ranked as given) against the scipy CSR `held`, the items
    of `train` at -inf; nan for a user with nothing held out."""
    s = masked(scores, train)
    held = held.tocsr()
    U = s.shape[0]
    tp = 1.0 / np.log2(np.arange(2, k + 2))
    recall, ndcg = np.full(U, np.nan), np.full(U, np.nan)
    for u in range(U):
        row = s[u]
        items = held.indices[held.indptr[u]:held.indptr[u + 1]]
        if len(items) == 0:
            continue
        hit = np.zeros(k, dtype=bool)
        for j in items:
            rank = int(np.sum(row > row[j]) + np.sum(row[:j] == row[j]))
            if rank < k:
                hit[rank] = True
        m = min(k, len(items))
        recall[u] = np.float64(np.float32(hit.sum())) / np.float64(m)
        ndcg[u] = np_pairwise_sum([tp[r] if hit[r] else 0.0 for r in range(k)]) / tp[:m].sum()
    return recall, ndcg


def decided(scores64, train, held, tau):
    """Users whose ranks an element error of at most `tau` cannot change: in the float64 scores no unmasked item other than j lies within
    2 tau of any held item j.  Users with nothing held out are not decided (they have no rank)."""
    s = masked(scores64, train)
    held = held.tocsr()
    out = np.zeros(s.shape[0], dtype=bool)
    for u in range(s.shape[0]):
        items = held.indices[held.indptr[u]:held.indptr[u + 1]]
        if len(items) == 0:
            continue
        row = s[u]
        ok = True
        for j in items:
            d = np.abs(row - row[j])   # (inf at the masked items)
            d[j] = np.inf
            ok = ok and not (d <= 2 * tau).any()
        out[u] = ok
    return out

"""The NeuMF downstream evaluator (reference: neural_cf_benchmark_pt.py): the module, its all-items ranking and the driver.

The reference trains NeuMF-end on (user, item, label) triples and, after every epoch and once at the end, pushes the cartesian product
of the validation users and the training items through the model in batches of 10000, merges the logits twice in pandas, rebuilds two
CSR matrices through Python dicts, densifies them and ranks.  Here that evaluation half has a device form: `Engine.neumf_scores`
(csrc/neumf.h) gives the dense logit matrix, `Engine.rank_metrics` masks and ranks it, `Engine.neumf_pair_logits` gives the per-epoch
validation loss.  The train loop is PyTorch by default; with `device_train=True` an epoch's batch loop is ONE `Engine.neumf_train_steps`
call (csrc/neumf_train.h: forward with dropout, loss, backward and Adam on the device), and with `device_draw=True` on top the epoch's
split, negatives and shuffle are ONE `Engine.neumf_epoch_draw` call on triples uploaded once (csrc/neumf_draw.h).  With `engine=None` the same functions run torch and numpy on the host - the checker.
The triples themselves - main.py:218-283's frames of a synthetic matrix's two tails and the split validation users - are stated once in
`synthetic_parts_host` / `assemble_triples`; `compute_neuralcf_results_synthetic` assembles them on the device instead, from CSR parts that
never leave it (`Engine.neumf_triples`, csrc/neumf_triples.h), and is what `pipeline.evaluate_synthetic` calls for hp["evaluator"] == "neumf";
with `device_ranking=True` the ranking problem is built from the same parts and its users selected on the device too
(`DeviceRankingProblem`, csrc/neumf_rank.h).

Triples are a numpy int array [n, 3] (user, item, label); a (user, item) pair occurs at most once per array.  Labels are taken as
binary (> 0), which is what the reference feeds its evaluators.  No pandas, no sklearn."""
from __future__ import annotations

import copy
import math

import numpy as np
import torch
import torch.nn as nn
from scipy.sparse import csr_matrix

K_LIST = (1, 3, 5, 10, 20, 50)
LR, BATCH, NUM_NEG, EARLY_STOP = 1e-3, 256, 1, 10            # :28-36, :255
EVAL_BATCH = 10000                                            # :224, :301 (host path)


class NCF(nn.Module):
    """NeuMF-end (:43-144 with model='NeuMF-end'): a GMF branch (elementwise product of two `factor`-wide embeddings) beside an MLP
    branch (two embeddings of factor * 2^(layers-1), concatenated, then `layers` times Dropout, Linear halving the width, ReLU), both
    concatenated into one Linear that gives the logit.  Parameter names, shapes and order are the reference's, so its checkpoints
    load; so is the initialisation (:84-100): N(0, 0.01) embeddings, Xavier-uniform tower, Kaiming-uniform (a=1, sigmoid gain) predict
    layer, zero biases."""

    def __init__(self, n_users, n_items, factor=8, layers=3, dropout=0.5):
        super().__init__()
        self.factor, self.layers = int(factor), int(layers)
        wide = self.factor * 2 ** (self.layers - 1)
        self.embed_user_GMF = nn.Embedding(n_users, self.factor)
        self.embed_item_GMF = nn.Embedding(n_items, self.factor)
        self.embed_user_MLP = nn.Embedding(n_users, wide)
        self.embed_item_MLP = nn.Embedding(n_items, wide)
        tower, width = [], 2 * wide
        for _ in range(self.layers):
            tower += [nn.Dropout(p=dropout), nn.Linear(width, width // 2), nn.ReLU()]
            width //= 2
        self.MLP_layers = nn.Sequential(*tower)
        self.predict_layer = nn.Linear(2 * self.factor, 1)
        for table in (self.embed_user_GMF, self.embed_user_MLP, self.embed_item_GMF, self.embed_item_MLP):
            nn.init.normal_(table.weight, std=0.01)
        for m in self.MLP_layers:
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
        nn.init.kaiming_uniform_(self.predict_layer.weight, a=1, nonlinearity="sigmoid")
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.zeros_(m.bias)

    def forward(self, user, item):
        gmf = self.embed_user_GMF(user) * self.embed_item_GMF(item)
        mlp = self.MLP_layers(torch.cat((self.embed_user_MLP(user), self.embed_item_MLP(item)), -1))
        return self.predict_layer(torch.cat((gmf, mlp), -1)).view(-1)

    def engine_weights(self, device=None):
        """The twelve tensors as `Engine.neumf_scores` takes them (`Engine.NEUMF_TENSORS` order): the live parameters themselves when
        they sit on `device` already, copies on it otherwise."""
        ts = [t.detach() for t in self.state_dict().values()]
        return ts if device is None else [t.to(device) for t in ts]


def _as_triples(a, name):
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != 3 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name}: an integer array [n, 3] of (user, item, label) triples is expected, got {a.dtype} {a.shape}")
    return a.astype(np.int64, copy=False)


def ranking_problem(training, heldout, users):
    """What the reference's testing block (:294-326) ranks, as index arrays: (users ascending and unique, columns = the item ids that occur
    in `training` ascending, relevant CSR [U, C] of the held-out triples with label > 0 whose item is a column, seen CSR [U, C] of every
    (user, item) pair of `training` whatever its label)."""
    training, heldout = _as_triples(training, "training"), _as_triples(heldout, "heldout")
    users = np.unique(np.asarray(users, dtype=np.int64))
    cols = np.unique(training[:, 1])

    def compact(t):
        keep = np.isin(t[:, 0], users) & np.isin(t[:, 1], cols)
        r, c = np.searchsorted(users, t[keep, 0]), np.searchsorted(cols, t[keep, 1])
        m = csr_matrix((np.ones(r.shape[0], dtype=np.float32), (r, c)), shape=(users.shape[0], cols.shape[0]))
        m.sum_duplicates()
        m.data[:] = 1.0
        m.sort_indices()
        return m
    return users, cols, compact(heldout[heldout[:, 2] > 0]), compact(training)


class RankingProblem:
    """`ranking_problem(training, heldout, users)` for any `users`, with the work that does not depend on them done ONCE: the columns,
    and both CSR matrices over every user id that occurs (rows by ascending id, columns sorted and unique).  `select(users)` is then a row
    selection - no `np.isin` over the triples, no CSR build - and returns what `ranking_problem` returns, array for array."""

    def __init__(self, training, heldout):
        training, heldout = _as_triples(training, "training"), _as_triples(heldout, "heldout")
        self.cols = np.unique(training[:, 1])
        self._relevant = self._rows(heldout[heldout[:, 2] > 0])
        self._seen = self._rows(training)

    def _rows(self, t):
        """(ids ascending and unique, indptr, indices) of the triples whose item is a column: per user id its distinct columns, ascending."""
        t = t[np.isin(t[:, 1], self.cols)]
        ids, r = np.unique(t[:, 0], return_inverse=True)
        m = csr_matrix((np.ones(t.shape[0], dtype=np.float32), (r.reshape(-1), np.searchsorted(self.cols, t[:, 1]))),
                       shape=(ids.shape[0], self.cols.shape[0]))
        m.sum_duplicates()
        m.sort_indices()
        return ids, m.indptr.astype(np.int64), m.indices

    @classmethod
    def from_parts(cls, parts, cols, heldout):
        """The object `RankingProblem(assemble_triples(parts)[0], heldout)` builds, array for array, from the parts' CSR patterns and
        `cols` - the ascending list of the item ids that occur in them (`flatnonzero` of `Engine.neumf_triples`' item_present) - without
        a triple array: a part's rows land at its user ids, a (user, item) pair that several parts hold is merged as `sum_duplicates`
        merges it.  `parts`: (scipy CSR pattern, user0, label) as `synthetic_parts_host` returns them."""
        self = cls.__new__(cls)
        self.cols = np.asarray(cols, dtype=np.int64)
        heldout = _as_triples(heldout, "heldout")
        self._relevant = self._rows(heldout[heldout[:, 2] > 0])
        top = max([int(user0) + m.shape[0] for m, user0, _ in parts] + [1])
        seen = csr_matrix((top, self.cols.shape[0]), dtype=np.float32)
        for m, user0, _ in parts:
            m = csr_matrix(m)
            m.sort_indices()
            counts = np.diff(m.indptr)
            keep = np.isin(m.indices, self.cols)
            r = np.repeat(np.arange(m.shape[0], dtype=np.int64) + int(user0), counts)[keep]
            c = np.searchsorted(self.cols, m.indices[keep])
            seen = seen + csr_matrix((np.ones(r.shape[0], dtype=np.float32), (r, c)), shape=seen.shape)
        seen.sum_duplicates()
        seen.sort_indices()
        ids = np.flatnonzero(np.diff(seen.indptr)).astype(np.int64)
        indptr = np.concatenate([[0], np.cumsum(np.diff(seen.indptr)[ids])]).astype(np.int64)
        self._seen = (ids, indptr, seen.indices)
        return self

    def _select(self, rows, users):
        ids, indptr, indices = rows
        start = length = np.zeros(users.shape[0], dtype=np.int64)
        if ids.shape[0]:
            at = np.minimum(np.searchsorted(ids, users), ids.shape[0] - 1)
            known = ids[at] == users                         # (an id that occurs nowhere: an empty row)
            start, length = np.where(known, indptr[at], 0), np.where(known, indptr[at + 1] - indptr[at], 0)
        out_ptr = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
        take = np.repeat(start - out_ptr[:-1], length) + np.arange(out_ptr[-1])
        return csr_matrix((np.ones(take.shape[0], dtype=np.float32), indices[take], out_ptr), shape=(users.shape[0], self.cols.shape[0]))

    def select(self, users):
        users = np.unique(np.asarray(users, dtype=np.int64))
        return users, self.cols, self._select(self._relevant, users), self._select(self._seen, users)


class DeviceRankingProblem:
    """The ranking problem resident on the engine's device (`Engine.neumf_rank_problem`, csrc/neumf_rank.h): the columns and both CSR
    matrices with their rows DENSE BY USER ID - row u is user u - so that a ranking's users need no row selection: `rank` hands their ids
    to `Engine.rank_metrics_rows` as a row map.  `rank_all_items(..., problem=<this>)` dispatches here."""

    def __init__(self, engine, record, n_items):
        self.engine, self.n_items = engine, int(n_items)
        self.cols, self.seen, self.relevant, self.counts = record.cols, record.seen, record.relevant, record.counts
        self.n_rows = int(self.seen[3][0])

    @classmethod
    def build(cls, engine, device_parts, n_items, item_present, validation, n_rows):
        """From what `compute_neuralcf_results_synthetic` holds behind `Engine.neumf_triples`: the same `device_parts` ((device CSR tuple,
        user0, label), ...), that call's `item_present`, the validation triples (an int array [n, 3], uploaded here once, or an int32
        device tensor) and the number of user ids (that call's counts[2]).  ONE `neumf_rank_problem` call; its 32 bytes of counts are all
        that comes back."""
        if not isinstance(validation, torch.Tensor):
            validation = torch.from_numpy(np.ascontiguousarray(_as_triples(validation, "validation"), dtype=np.int32)).to(engine.device)
        return cls(engine, engine.neumf_rank_problem(device_parts, n_items, item_present, validation, n_rows), n_items)

    def to_host(self):
        """The `RankingProblem` that `RankingProblem.from_parts` builds from the same parts, array for array (tests and debugging only: it
        reads everything back)."""
        host = RankingProblem.__new__(RankingProblem)
        host.cols = self.cols.cpu().numpy().astype(np.int64)

        def rows(csr_dev):
            indptr, indices = csr_dev[0].cpu().numpy(), csr_dev[1].cpu().numpy()
            lengths = np.diff(indptr)
            ids = np.flatnonzero(lengths).astype(np.int64)
            return ids, np.concatenate([[0], np.cumsum(lengths[ids])]).astype(np.int64), indices[:indptr[-1]].astype(np.int32)
        host._relevant, host._seen = rows(self.relevant), rows(self.seen)
        return host

    def rank(self, model, users):
        """`rank_all_items`' result for `users`: the uint8 device mask [n_rows] that `Engine.neumf_epoch_draw` leaves in `present`
        (compacted on the device, `Engine.neumf_rank_users`), or an array of ids (made unique on the host and uploaded: the final
        ranking's few hundred validation users)."""
        engine = self.engine
        if int(self.cols.numel()) <= max(K_LIST):
            raise ValueError(f"ranking needs more than {max(K_LIST)} training items, got {int(self.cols.numel())}")
        if isinstance(users, torch.Tensor) and users.dtype == torch.uint8:
            users_dev = engine.neumf_rank_users(users)
        else:
            users = users.cpu().numpy() if isinstance(users, torch.Tensor) else users
            users_dev = torch.from_numpy(np.unique(np.asarray(users, dtype=np.int64)).astype(np.int32)).to(engine.device)
        if users_dev.numel() == 0:
            return np.empty((len(K_LIST), 0)), np.empty((len(K_LIST), 0))
        scores = engine.neumf_scores(model.engine_weights(engine.device), users_dev, self.cols, check=False)
        rec, ndcg = engine.rank_metrics_rows(scores, users_dev, self.relevant, self.seen, ks=K_LIST, full_idcg=True)
        rec, ndcg = rec.cpu().numpy(), ndcg.cpu().numpy()
        engine.feed_status()
        return rec, ndcg


def synthetic_parts_host(train_shape, valid, ones, zeros):
    """What main.py:218-283 hands to `compute_neuralcf_results` for ONE synthetic matrix in its non-augmented branch
    (`args.augment_training_data` false, `data = equal_sparsity_valid_train`, :279-280 - the branch the `mlp` route takes too), as
    (parts, validation): `parts` a list of (scipy CSR pattern, user0, label) whose triples - `assemble_triples(parts)` - are the training
    frame, `validation` the int64 [n, 3] validation triples.
      * `zeros`, the lower tail `raw <= quantile(raw, 1 - sparsity)` (:259-262, :270): label 0, user = row with NO offset - :275 builds the
        training frame before :277 adds TRAIN_DATA.shape[0] + VALID_DATA.shape[0] to the users, and that is kept;
      * `ones`, the upper tail `raw >= quantile(raw, sparsity)` (:258-261, :267): label 1, user = row;
      * valid_train, valid_test = `metrics.split_train_test_proportion_from_csr_matrix(valid.copy(), batch_size=10, random_seed=123,
        ignore_zeros=True)` (:226-228; it renumbers the users it keeps, those with two entries or more): valid_train's entries get label 1
        and user = row + train_shape[0] (:230-233); the validation triples are valid_test's entries, row-major, the same offset, label 1
        (:235-237).
    The parts come in the order zeros, ones, valid_train (:273-275).  NOT reproduced, on purpose:
      * the reference shuffles the frames with a fixed pandas seed (`sample(frac=1, random_state=123)`, :240, :246, :273, :275): every
        consumer here shuffles per epoch, so the order is `assemble_triples`' and no pandas draw is made;
      * the halves of the "stored zeros of VALID_DATA" (:240-249) are empty for every dataset the project loads (binarised CSR matrices
        store no zero); a `valid` with a stored value other than 1 is refused rather than guessed at;
      * the augmented branch (:251-254 `train_data[~train_data.isin(valid_data)]`, :278) is not built;
      * the reference's M arm thresholds F_SDRM once more (:287-291), so its "M" figure is F's: here each tag evaluates its own matrix."""
    from . import metrics
    valid = csr_matrix(valid)
    if valid.nnz and np.any(valid.data != 1):
        raise ValueError("synthetic_parts_host: `valid` stores a value other than 1; main.py:242 would send its stored zeros, shuffled by pandas, "
                         "into both frames, which is not reproduced")
    valid_train, valid_test = metrics.split_train_test_proportion_from_csr_matrix(valid.copy(), batch_size=10, random_seed=123, ignore_zeros=True)
    offset = int(train_shape[0])

    def pattern(m):
        m = csr_matrix(m)
        m.sort_indices()
        return m
    valid_test = pattern(valid_test)
    users = np.repeat(np.arange(valid_test.shape[0], dtype=np.int64), np.diff(valid_test.indptr)) + offset
    validation = np.stack([users, valid_test.indices.astype(np.int64), np.ones(users.shape[0], dtype=np.int64)], axis=1)
    return [(pattern(zeros), 0, 0), (pattern(ones), 0, 1), (pattern(valid_train), offset, 1)], validation


def assemble_triples(parts):
    """The host form of sdrm_neumf_triples' order (include/sdrm_hip.h): (triples int64 [m, 3], (n_users, n_items)) of (scipy CSR pattern,
    user0, label) parts - the parts in the order given, rows ascending, a row's entries in their stored order; n_users = max user + 1 and
    n_items = max item + 1 over the triples, as main.py:283 takes them (0, 0 without a triple)."""
    out = []
    for m, user0, label in parts:
        users = np.repeat(np.arange(m.shape[0], dtype=np.int64), np.diff(m.indptr)) + int(user0)
        out.append(np.stack([users, m.indices[m.indptr[0]:m.indptr[-1]].astype(np.int64), np.full(users.shape[0], int(label), dtype=np.int64)], axis=1))
    triples = np.concatenate(out) if out else np.zeros((0, 3), dtype=np.int64)
    dims = (int(triples[:, 0].max()) + 1, int(triples[:, 1].max()) + 1) if triples.shape[0] else (0, 0)
    return triples, dims


def _idcg_table():
    tp = 1.0 / np.log2(np.arange(2, max(K_LIST) + 2))
    return tp, np.asarray([tp[:m].sum() for m in range(max(K_LIST) + 1)])


def host_metrics(scores, relevant):
    """Per-user (recall [6, U], ndcg [6, U]) of masked scores [U, C] (float, -inf where seen) against the boolean `relevant` [U, C], the way
    utilities.recall_at_k_batch / NDCG_binary_at_k_batch come out on the CSR matrices the reference builds: its held-out matrix stores an
    explicit entry for EVERY pair of the cartesian product, so `getnnz` is the column count and the ideal DCG is sum(tp[:min(C, k)]) for
    every user; a user without a relevant item has recall nan (0 / 0) and NDCG 0."""
    U, C = scores.shape
    if C <= max(K_LIST):
        raise ValueError(f"ranking needs more than {max(K_LIST)} columns, got {C}")
    tp, idcg = _idcg_table()
    rows = np.arange(U)[:, None]
    n_true = relevant.sum(axis=1)
    recall, ndcg = np.empty((len(K_LIST), U)), np.empty((len(K_LIST), U))
    for q, k in enumerate(K_LIST):
        part = np.argpartition(-scores, k, axis=1)[:, :k]
        topk = part[rows, np.argsort(-scores[rows, part], axis=1)]
        hits = relevant[rows, part].sum(axis=1).astype(np.float32)
        with np.errstate(invalid="ignore", divide="ignore"):
            recall[q] = hits / np.minimum(k, n_true)
        ndcg[q] = (relevant[rows, topk] * tp[:k]).sum(axis=1) / idcg[min(C, k)]
    return recall, ndcg


@torch.no_grad()
def host_scores(model, users, items):
    """The logits of every listed user against every listed item from the torch module in eval mode, in the reference's batches of 10000
    pairs (:219-233): float32 numpy [U, C]."""
    device = next(model.parameters()).device
    was_training = model.training
    model.eval()
    pairs = torch.cartesian_prod(torch.as_tensor(users, dtype=torch.int32, device=device), torch.as_tensor(items, dtype=torch.int32, device=device))
    out = [model(pairs[s:s + EVAL_BATCH, 0], pairs[s:s + EVAL_BATCH, 1]) for s in range(0, pairs.shape[0], EVAL_BATCH)]
    model.train(was_training)
    return torch.cat(out).reshape(len(users), len(items)).cpu().numpy()


def rank_all_items(model, training, heldout, users, engine=None, problem=None):
    """The reference's testing block (:294-332; the per-epoch one :215-246 is the same) for `model`: per-user (recall [6, U], ndcg [6, U])
    float64 numpy arrays for `K_LIST`, row q of either for the q-th smallest id in `users`.  As the reference behaves:
      * the columns are the item ids that occur in `training`; a held-out item that never occurs there is dropped;
      * every (user, item) pair present in `training`, with any label, 0 included, is masked to -inf;
      * only held-out triples with label > 0 are relevant;
      * the ideal DCG counts min(columns, k) items for every user (see `host_metrics`); a user without a relevant item: recall nan, NDCG 0.
    With an engine the two CSR matrices are compacted here with numpy and uploaded, the logits are ONE `neumf_scores` call, masking and
    ranking are the existing `rank_metrics`; its NDCG (ideal DCG of min(relevant, k) items, nan without one) is put on the reference's
    footing from the per-user counts on the host.  `feed_status()` is asked once.  Without one, torch and numpy do all of it.
    `problem`: a `RankingProblem(training, heldout)` of the same two arrays, built once by a caller that ranks more than once; the index
    arrays are then a row selection from it, the same as `ranking_problem`'s.  A `DeviceRankingProblem` (needs its engine) ranks without
    one: `users` is then the uint8 device mask of the users or an id array, both matrices stay on the device and are read through a row
    map (`DeviceRankingProblem.rank`: ONE `neumf_scores` call, `Engine.rank_metrics_rows(..., full_idcg=True)` - the footing made on the
    device in the host's three operations - and `feed_status()` once), and the result is the same pair of arrays."""
    if isinstance(problem, DeviceRankingProblem):
        if engine is None or engine is not problem.engine:
            raise ValueError("rank_all_items: a DeviceRankingProblem ranks on the engine that built it")
        return problem.rank(model, users)
    users, cols, relevant, seen = ranking_problem(training, heldout, users) if problem is None else problem.select(users)
    if cols.shape[0] <= max(K_LIST):
        raise ValueError(f"ranking needs more than {max(K_LIST)} training items, got {cols.shape[0]}")
    if engine is None:
        scores = host_scores(model, users, cols).astype(np.float32)
        scores[seen.nonzero()] = -np.inf
        return host_metrics(scores, relevant.toarray() > 0)
    weights = model.engine_weights(engine.device)
    scores = engine.neumf_scores(weights, torch.from_numpy(users.astype(np.int32)).to(engine.device),
                                 torch.from_numpy(cols.astype(np.int32)).to(engine.device), check=False)
    rec, ndcg = engine.rank_metrics(scores, engine.csr_to_device(relevant), engine.csr_to_device(seen), ks=K_LIST)
    rec, ndcg = rec.cpu().numpy(), ndcg.cpu().numpy()
    engine.feed_status()
    _, idcg = _idcg_table()
    n_true = np.diff(relevant.indptr)
    for q, k in enumerate(K_LIST):
        ndcg[q] = np.where(n_true > 0, ndcg[q] * idcg[np.minimum(n_true, k)] / idcg[min(cols.shape[0], k)], 0.0)
    return rec, ndcg


def _bce_with_logits(logits, labels):
    return nn.functional.binary_cross_entropy_with_logits(logits, labels)


def validation_loss(model, triples, engine=None):
    """`BCEWithLogitsLoss` of the model in eval mode on (user, item, label) triples (:203-211) as a Python float: `neumf_pair_logits`'s
    loss sum over n with an engine, torch's own on the model's device without.  With an engine `triples` may also be an int32 tensor
    [n, 3] on the engine's device (the hold-out part `Engine.neumf_epoch_draw` leaves): its columns become contiguous device arrays with
    torch ops, nothing is uploaded, and the divisor is n."""
    if isinstance(triples, torch.Tensor):
        if engine is None:
            raise ValueError("validation_loss: device triples need an engine (the host form takes the numpy array)")
        if triples.dtype != torch.int32 or triples.dim() != 2 or triples.shape[1] != 3 or triples.device != engine.device:
            raise ValueError(f"validation_loss: device triples must be an int32 tensor [n, 3] on {engine.device}, got {triples.dtype} {tuple(triples.shape)} on {triples.device}")
        _, loss_sum = engine.neumf_pair_logits(model.engine_weights(engine.device), triples[:, 0].contiguous(), triples[:, 1].contiguous(),
                                               triples[:, 2].to(torch.float32).contiguous(), check=False)
        return float(loss_sum.item()) / triples.shape[0]
    triples = _as_triples(triples, "triples")
    if engine is not None:
        dev = engine.device
        _, loss_sum = engine.neumf_pair_logits(model.engine_weights(dev), torch.from_numpy(triples[:, 0].astype(np.int32)).to(dev),
                                               torch.from_numpy(triples[:, 1].astype(np.int32)).to(dev),
                                               torch.from_numpy(triples[:, 2].astype(np.float32)).to(dev), check=False)
        return float(loss_sum.item()) / triples.shape[0]
    device = next(model.parameters()).device
    was_training = model.training
    model.eval()
    with torch.no_grad():
        x = torch.as_tensor(triples, dtype=torch.int32, device=device)
        loss = _bce_with_logits(model(x[:, 0], x[:, 1]), x[:, 2].float()).item()
    model.train(was_training)
    return loss


def compute_neuralcf_results(training, validation, n_users, n_items, engine=None, seed=0, epochs=20, eval_recall=True, device=None,
                             history=None, device_train=False, device_draw=False):
    """The reference's driver (:154-334) over int triples [n, 3]: (recall [6], ndcg [6]) for `K_LIST`, nanmean over the validation users
    rounded to 4 places.  As the reference: NCF(factor 8, three layers, dropout 0.5), Adam(1e-3), BCEWithLogitsLoss, batches of 256; per
    epoch a fresh 80/20 split of `training`, as many label-0 rows of the 80 % drawn again WITH replacement as it has label-1 rows
    (num_neg = 1), everything shuffled; after the epoch the loss on the 20 % and, with `eval_recall`, Recall@10 of the 20 %'s users
    against `validation`.  Which weights rank at the end is the reference's too: without `eval_recall` those of the epoch with the lowest
    validation loss; with it those of EPOCH 0 (the reference saves every epoch that improves Recall@10 but loads `best_epoch`, which
    that branch never sets).  Where epoch 0's Recall@10 was 0 or nan the reference has no file of this run to load - it fails, or loads a
    stale file of an earlier run; THIS driver's own choice there, not the reference's, is to rank with the last epoch's weights, and
    `history` says so ('best_epoch' is then that last epoch and 'reference_has_no_checkpoint' is True).
    The early-stop counter runs as the reference's does (with `eval_recall` it is never reset) and stops the loop at 10.  Weights are
    kept in memory, not in a directory.
    The reference's shuffles are unseeded; here every draw comes from `numpy.random.default_rng(seed)` (split permutation, negative
    draw, shuffle, in that order per epoch), the module's initialisation and its dropout from torch's GLOBAL generator, seeded with
    `seed` on entry (`torch.manual_seed`): numpy's global generator is not touched, torch's is left wherever training took it.
    The train loop is torch in both modes and runs on `device` (default: the engine's device, the CPU without one).  With an engine the
    per-epoch validation loss is `neumf_pair_logits`, both rankings are `rank_all_items(..., engine)`, and `feed_status()` is asked once
    per evaluation; weights that live elsewhere than on the engine's device are copied there per evaluation.
    `device_train=True` (needs an engine; the model then lives on the engine's device) replaces the batch loop :186-200 of every epoch by
    ONE `Engine.neumf_train_steps` call: the shuffled triples are uploaded as int32 once per epoch, Adam's moments are twelve zero tensors
    made once and its step count runs on across the epochs, no torch optimizer exists and no autograd runs.  The split, the negatives, the
    shuffle, the early stop and which weights rank are untouched - but the DROPOUT draws are then the engine's Philox4x32-10 of
    (seed, epoch, the triple's place in the epoch's array, column), not torch's generator, so the trained weights differ from the torch
    loop's as two seeds of it differ.  `history` then also receives 'train_loss': every step's loss, read back once per epoch.
    `device_draw=True` (needs `device_train=True` and an engine) moves the epoch's data preparation to the device as well: `training` is
    cast to int32 and uploaded ONCE per call, and per epoch ONE `Engine.neumf_epoch_draw(seed=seed, epoch=epoch)` fills device buffers
    with the split, the negatives and the shuffle - the draw defined in include/sdrm_hip.h at sdrm_neumf_epoch_draw (keyed Feistel
    permutations of Philox4x32-10, restated in tests/neumf_draw_ref.py).  `neumf_train_steps` reads the shuffled part in place, the
    validation loss reads the device-resident hold-out part, and the epoch's users come from n_users bytes read back.  Sizes, the
    condition for the negatives (label-1 and label-0 rows both present) and everything behind the draw are untouched - but the draws are
    then a function of (seed, epoch) alone and `numpy.random.default_rng(seed)` is not consumed, so the trained weights differ from the
    host-draw path's as two seeds of it differ.  Torch's global generator is seeded and used for the initialisation as in every mode.
    `history` then also receives 'draw_counts': one (n_pos, n_neg, m) per epoch.
    In every mode the ranking problem (columns and both CSR matrices) is built once per call (`RankingProblem`) and the per-epoch and
    final rankings select their users' rows from it: the same index arrays as before, without the per-epoch rebuild.
    `history`: a dict that receives 'valid_loss' (per epoch), 'recall10' (per epoch, with eval_recall), 'best_epoch' (the epoch whose
    weights ranked), 'reference_has_no_checkpoint', 'best_recall_epoch', 'epochs_run', 'per_user' (the final per-user recall / ndcg)
    and 'model' (the module that ranked)."""
    return compute_neuralcf_results_resident(training, validation, n_users, n_items, engine=engine, seed=seed, epochs=epochs, eval_recall=eval_recall,
                                             device=device, history=history, device_train=device_train, device_draw=device_draw)


def compute_neuralcf_results_resident(training, validation, n_users, n_items, engine=None, seed=0, epochs=20, eval_recall=True, device=None,
                                      history=None, device_train=False, device_draw=False, training_dev=None, problem=None):
    """`compute_neuralcf_results` - its body: that function is this one with the last two arguments left out, and everything its docstring
    says holds here - with two more keyword arguments for a caller whose training triples are on the device already.
    `training_dev` and `problem` (both None by default; either one needs `device_draw=True` and raises ValueError without it, and they come together): the training triples
    as an int32 tensor [n, 3] already on the engine's device - `Engine.neumf_triples`' view - used in place of the cast and upload, and a
    `RankingProblem` of the same triples (`RankingProblem.from_parts`) used in place of `RankingProblem(training, validation)` - or a
    `DeviceRankingProblem` of them (`DeviceRankingProblem.build`), with which an epoch's users are `present` itself, never read back.
    `training` may then be None: nothing else reads it, and the hold-out size comes from `training_dev.shape[0]`.
    They are their own function because `compute_neuralcf_results`' parameter list is pinned by tests/test_neumf_epoch_draw_host.py."""
    if (training_dev is not None or problem is not None) and not device_draw:
        raise ValueError("compute_neuralcf_results_resident: training_dev and problem stand in for the upload and the ranking problem of device_draw=True; "
                         "without it the host draws from `training`")
    resident = training_dev is not None and problem is not None
    if (training_dev is None) != (problem is None):
        raise ValueError("compute_neuralcf_results_resident: training_dev and problem come together (the ranking problem of the device triples)")
    if training is None and not resident:
        raise ValueError("compute_neuralcf_results: training is None; only training_dev with problem (device_draw=True) can stand in for it")
    validation = _as_triples(validation, "validation")
    if training is not None:
        training = _as_triples(training, "training")
    if device_draw and (engine is None or not device_train):
        raise ValueError("compute_neuralcf_results: device_draw=True needs device_train=True and an engine (the draw fills device buffers that the "
                         "device train step reads in place; there is no host form)")
    device = torch.device(device) if device is not None else (engine.device if engine is not None else torch.device("cpu"))
    if device_train:
        if engine is None:
            raise ValueError("compute_neuralcf_results: device_train=True needs an engine (the train step runs on the device; there is no host form)")
        if device != engine.device:
            raise ValueError(f"compute_neuralcf_results: device_train=True trains on the engine's device {engine.device}, not on {device}")
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    model = NCF(n_users, n_items, factor=8, layers=3, dropout=0.5).to(device)
    train_losses, steps_done = [], 0
    if device_train:
        live = model.engine_weights()                        # the parameters themselves: the engine updates them in place
        exp_avg, exp_avg_sq = [torch.zeros_like(t) for t in live], [torch.zeros_like(t) for t in live]
    else:
        optimizer = torch.optim.Adam(model.parameters(), lr=LR)
    best_loss, best_epoch, best_recall, best_recall_epoch, early_stop = math.inf, 0, 0.0, None, 0
    kept = {0: None}
    valid_losses, recalls, epochs_run = [], [], 0
    n_train = int(training_dev.shape[0]) if resident else training.shape[0]
    n_hold = int(math.ceil(0.2 * n_train))                    # sklearn's train_test_split(test_size=0.2): ceil for the test part
    if not resident:
        problem = RankingProblem(training, validation)
    draw_counts = []
    if device_draw:
        if not resident:
            training_dev = torch.from_numpy(np.ascontiguousarray(training, dtype=np.int32)).to(device)
        draw_bufs = (torch.empty(n_hold, 3, dtype=torch.int32, device=device),
                     torch.empty(2 * (n_train - n_hold), 3, dtype=torch.int32, device=device))
    for epoch in range(epochs):
        epochs_run += 1
        model.train()
        if device_draw:
            hold, triples_dev, counts, present = engine.neumf_epoch_draw(training_dev, n_hold, seed=seed, epoch=epoch, out=draw_bufs,
                                                                         n_users=n_users if eval_recall else None)   # (`present` only where a ranking reads it)
            draw_counts.append(counts)
        else:
            perm = rng.permutation(training.shape[0])
            hold, part = training[perm[:n_hold]], training[perm[n_hold:]]
            negatives = part[part[:, 2] == 0]
            n_pos = int((part[:, 2] == 1).sum())
            if n_pos and negatives.shape[0]:
                part = np.concatenate([part, negatives[rng.integers(0, negatives.shape[0], size=n_pos * NUM_NEG)]])
            part = part[rng.permutation(part.shape[0])]
        if device_train:
            if not device_draw:
                triples_dev = torch.from_numpy(np.ascontiguousarray(part, dtype=np.int32)).to(device)
            losses = engine.neumf_train_steps(live, exp_avg, exp_avg_sq, triples_dev, BATCH, steps_done, lr=LR, p_drop=0.5, seed=seed, call_id=epoch,
                                              check=False)     # (the evaluation below asks feed_status)
            steps_done += int(losses.numel())
            train_losses.extend(losses.cpu().tolist())
        for s in () if device_train else range(0, part.shape[0], BATCH):
            x = torch.as_tensor(part[s:s + BATCH], dtype=torch.int32, device=device)
            model.zero_grad()
            loss = _bce_with_logits(model(x[:, 0], x[:, 1]), x[:, 2].float())
            loss.backward()
            optimizer.step()
        model.eval()
        valid_loss = validation_loss(model, hold, engine)
        valid_losses.append(valid_loss)
        if eval_recall:
            if isinstance(problem, DeviceRankingProblem):
                epoch_users = present                          # the mask itself: compacted, scored and ranked on the device
            else:
                epoch_users = np.flatnonzero(present.cpu().numpy()) if device_draw else hold[:, 0]
            rec, _ = rank_all_items(model, training, validation, epoch_users, engine, problem=problem)
            with np.errstate(invalid="ignore"):
                recall10 = float(np.nanmean(rec[K_LIST.index(10)])) if rec.shape[1] else float("nan")
            recalls.append(recall10)
            if recall10 > best_recall:
                # The reference notes this epoch in `best_recall_epoch` and saves its weights, but loads `best_epoch` at the end, which
                # this branch never sets: what it loads is epoch 0's file.  So only epoch 0's weights are ever needed here.
                best_recall, best_recall_epoch, best_loss = recall10, epoch, valid_loss
                if epoch == 0:
                    kept = {0: copy.deepcopy(model.state_dict())}
            else:
                early_stop += 1
        else:
            if engine is not None:
                engine.feed_status()          # (with eval_recall the ranking above has asked)
            if best_loss > valid_loss:
                best_loss, best_epoch, early_stop = valid_loss, epoch, 0
                kept = {epoch: copy.deepcopy(model.state_dict())}
            else:
                early_stop += 1
        if early_stop == EARLY_STOP:
            break
    no_checkpoint = kept.get(best_epoch) is None
    if no_checkpoint:
        best_epoch = epochs_run - 1       # nothing of this run to load: the live weights rank, and the history names their epoch
    else:
        model.load_state_dict(kept[best_epoch])
    model.eval()
    rec, ndcg = rank_all_items(model, training, validation, validation[:, 0], engine, problem=problem)
    if history is not None:
        history.update(valid_loss=valid_losses, recall10=recalls, best_epoch=best_epoch, reference_has_no_checkpoint=no_checkpoint, best_recall_epoch=best_recall_epoch, epochs_run=epochs_run, per_user=(rec, ndcg), model=model)
        if device_train:
            history["train_loss"] = train_losses
        if device_draw:
            history["draw_counts"] = draw_counts
    with np.errstate(invalid="ignore"):
        return (np.array([np.round(np.nanmean(rec[q]), 4) for q in range(len(K_LIST))]),
                np.array([np.round(np.nanmean(ndcg[q]), 4) for q in range(len(K_LIST))]))


def compute_neuralcf_results_synthetic(train_shape, valid, raw, sparsity, engine, seed=0, epochs=20, eval_recall=True, history=None,
                                       device_ranking=False):
    """main.py's NeuMF arm for ONE synthetic matrix `raw` (dense scores, on the engine's device or the host; main.py:256-283, the
    non-augmented branch - see `synthetic_parts_host` for what is kept and what is not) with the training triples ASSEMBLED ON THE
    DEVICE: both tails come from `Engine.equal_sparsity_csr` and stay resident, the validation users' training half
    (`synthetic_parts_host`'s split, a few hundred users) is uploaded with `csr_to_device`, ONE `Engine.neumf_triples` call writes the
    triples into the buffer `neumf_epoch_draw` reads, and `compute_neuralcf_results_resident(None, validation, n_users, n_items, engine,
    device_train=True, device_draw=True, training_dev=..., problem=...)` trains and ranks; n_users and n_items are the call's counts
    (max user + 1, max item + 1: main.py:283).  Neither the dense 0/1 matrix nor the triples cross to the host.  What does cross: 32 bytes
    of counts, n_items bytes of `item_present` (the ranking's columns) and, once, the two tails' indptr / indices, from which
    `RankingProblem.from_parts` builds the host-side ranking problem.
    `device_ranking=True` builds the ranking problem on the device instead (`DeviceRankingProblem.build`: ONE `Engine.neumf_rank_problem`
    call from the same parts, `item_present`, the call's user count and the validation triples, uploaded once): the tails are not read
    back, `from_parts` is not called, and per ranking the epoch's `present` mask is compacted, scored and ranked on the device.  What
    crosses then: the counts (32 bytes twice), 8 bytes per ranking (the number of its users) and the per-user metrics, 2 x 6 x U doubles."""
    if engine is None:
        raise ValueError("compute_neuralcf_results_synthetic: needs an engine (the host form is compute_neuralcf_results on "
                         "assemble_triples(synthetic_parts_host(...)))")
    n_items = int(raw.shape[1])
    ones_dev = engine.equal_sparsity_csr(raw, float(sparsity), side=">=")
    zeros_dev = engine.equal_sparsity_csr(raw, 1.0 - float(sparsity), side="<=")
    empty = csr_matrix((int(raw.shape[0]), n_items), dtype=np.float32)
    parts, validation = synthetic_parts_host(train_shape, valid, empty, empty)   # (the split and the validation triples; the tails stay on the device)
    valid_train, offset, _ = parts[2]
    device_parts = [(zeros_dev, 0, 0), (ones_dev, 0, 1)]
    if valid_train.shape[0]:
        device_parts.append((engine.csr_to_device(valid_train), offset, 1))
    training_dev, counts, item_present = engine.neumf_triples(device_parts, n_items)
    if device_ranking:
        problem = DeviceRankingProblem.build(engine, device_parts, n_items, item_present, validation, counts[2])
        return compute_neuralcf_results_resident(None, validation, counts[2], counts[3], engine=engine, seed=seed, epochs=epochs, eval_recall=eval_recall,
                                                 history=history, device_train=True, device_draw=True, training_dev=training_dev, problem=problem)

    def host_pattern(dev):
        indptr, indices, shape = dev
        indptr, indices = indptr.cpu().numpy(), indices.cpu().numpy()
        return csr_matrix((np.ones(indices.shape[0], dtype=np.float32), indices, indptr), shape=shape)
    host_parts = [(host_pattern(zeros_dev), 0, 0), (host_pattern(ones_dev), 0, 1), (valid_train, offset, 1)]
    problem = RankingProblem.from_parts(host_parts, np.flatnonzero(item_present.cpu().numpy()), validation)
    return compute_neuralcf_results_resident(None, validation, counts[2], counts[3], engine=engine, seed=seed, epochs=epochs, eval_recall=eval_recall,
                                             history=history, device_train=True, device_draw=True, training_dev=training_dev, problem=problem)

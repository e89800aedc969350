#!/usr/bin/env python3
"""Generate tests/golden/neumf_eval.npz from the upstream reference (CPU, where the reference exists; see make_golden.py).

The reference's own `NCF(..., model='NeuMF-end').eval()` (neural_cf_benchmark_pt.py:43-144) with the injected tensors of
tests/neumf_ref.py::weights, on the inputs its case tables rebuild from seeds.  Stored:
  <case>_logits     the reference's float32 logits [users, items] for every row of neumf_ref.CASES;
  loss_logits, loss_value   its logits for the loss case's pairs and its `BCEWithLogitsLoss` of them (float32);
  quirk_logits, quirk_recall, quirk_ndcg   for the ranking case neumf_ref.QUIRK: its logits for the cartesian product its testing block
                    (:294-332) scores, and the per-user Recall@k / NDCG@k [6, users] that `utilities.recall_at_k_batch` and
                    `utilities.NDCG_binary_at_k_batch` give on the two CSR matrices `utilities.create_csr_from_df` builds from the merged
                    frame (the merges are restated here with pandas; the three functions are the reference's);
  <rank case>_dev   the normwise deviation of the reference's float32 logits from the float64 oracle on each ranking case.
The inputs themselves are not stored.  The conditions tests/test_neumf_eval.py puts on the ranking cases are asserted here as well.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_neumf_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pandas as pd   # before load_reference() stubs `bottleneck`: pandas looks for the real one when it is imported

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import load_reference  # noqa: E402
import torch  # noqa: E402
import neumf_ref as nr  # noqa: E402

BAR_FACTOR, GAP_FACTOR, EXEMPT_SHARE = 4.0, 8.0, 0.02   # tests/test_neumf_eval.py


def upstream_model(up, w):
    n_users, F = w[nr.NAMES[0]].shape
    model = up.NCF(n_users, w[nr.NAMES[1]].shape[0], F, 3, 0.5, "NeuMF-end").eval()
    assert list(model.state_dict()) == list(nr.NAMES)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return model


def upstream_scores(model, users, items):
    with torch.no_grad():
        pairs = torch.cartesian_prod(torch.tensor(users, dtype=torch.int32), torch.tensor(items, dtype=torch.int32))
        return model(pairs[:, 0], pairs[:, 1]).numpy().reshape(len(users), len(items)).astype(np.float32)


def upstream_ranking(utilities, users, cols, logits, training, heldout):
    """The frame of the testing block: one row per (user, item) of the product with the prediction, the held-out label (0 where the
    pair is not held out) and the prediction masked to -inf where the pair occurs in training; then the reference's functions."""
    uu, ii = np.meshgrid(users, cols, indexing="ij")
    frame = pd.DataFrame({0: uu.ravel(), 1: ii.ravel()})
    frame["predictions"] = logits.ravel().astype(np.float64)
    frame["validation_labels"] = frame.merge(pd.DataFrame(heldout), on=[0, 1], how="left")[2].fillna(0)
    frame["training_labels"] = frame.merge(pd.DataFrame(training), on=[0, 1], how="left")[2]
    frame["masked_predictions"] = frame["predictions"].where(frame["training_labels"].isnull(), other=-np.inf)
    actual = utilities.create_csr_from_df(frame, user_col=0, item_col=1, rating_col="validation_labels")[0]
    pred = utilities.create_csr_from_df(frame, user_col=0, item_col=1, rating_col="masked_predictions")[0]
    recall = np.stack([utilities.recall_at_k_batch(pred.toarray(), actual, k=k) for k in nr.K_LIST])
    ndcg = np.stack([utilities.NDCG_binary_at_k_batch(pred.toarray(), actual, k=k) for k in nr.K_LIST])
    return recall.astype(np.float64), ndcg.astype(np.float64)


def main():
    load_reference()
    import neural_cf_benchmark_pt as up  # type: ignore
    import utilities  # type: ignore

    out = {}
    for name in nr.CASES:
        w, users, items, _ = nr.case_inputs(name)
        logits = upstream_scores(upstream_model(up, w), users, items)
        out[f"{name}_logits"] = logits
        print(name, logits.shape, "fp32 deviation", nr.normwise(logits, nr.scores64(w, users, items)))

    w, users, items, labels = nr.loss_inputs()
    with torch.no_grad():
        x = upstream_model(up, w)(torch.from_numpy(users), torch.from_numpy(items))
        out["loss_logits"] = x.numpy().astype(np.float32)
        out["loss_value"] = np.asarray(torch.nn.BCEWithLogitsLoss()(x, torch.from_numpy(labels)).item(), dtype=np.float32)
    x64 = nr.forward64(w, users, items)
    for y in (0.0, 1.0):
        assert (x64[labels == y] > 18).any() and (x64[labels == y] < -18).any(), "the loss case must reach |x| ~ 20 on both sides of each label"
    print("loss", out["loss_value"], "float64", nr.bce64(x64, labels))

    for name in nr.RANK_CASES:
        w, training, heldout = nr.rank_inputs(name)
        users, cols, relevant, seen = nr.rank_problem(training, heldout)
        logits = upstream_scores(upstream_model(up, w), users, cols)
        ref = nr.scores64(w, users, cols)
        dev = nr.normwise(logits, ref)
        out[f"{name}_dev"] = np.asarray(dev)
        fewest, exempt = nr.rank_conditions(ref, relevant, seen, GAP_FACTOR * BAR_FACTOR * dev * np.abs(ref).max())
        assert fewest >= max(nr.K_LIST) + 1, (name, fewest)
        assert len(exempt) <= EXEMPT_SHARE * len(users), (name, exempt)
        print(name, ref.shape, "fp32 deviation", dev, "fewest unmasked columns", fewest, "exempt users", exempt)
        if name == nr.QUIRK:
            recall, ndcg = upstream_ranking(utilities, users, cols, logits, training, heldout)
            no_positive = np.flatnonzero(relevant.sum(axis=1) == 0)
            assert no_positive.size and np.isnan(recall[:, no_positive]).all() and (ndcg[:, no_positive] == 0).all()
            assert not np.isin(heldout[heldout[:, 2] > 0, 1], cols).all(), "a held-out item absent from training"
            assert ((training[:, 2] == 0) & np.isin(training[:, 0], users)).any(), "a label-0 training pair of a ranked user"
            assert (relevant.sum(axis=1) < 10).all(), "fewer relevant items than k"
            ref_recall, ref_ndcg = nr.rank_metrics64(logits, relevant, seen)
            assert np.allclose(ref_recall, recall, rtol=0, atol=1e-12, equal_nan=True) and np.allclose(ref_ndcg, ndcg, rtol=0, atol=1e-12)
            out["quirk_logits"], out["quirk_recall"], out["quirk_ndcg"] = logits, recall, ndcg
    path = os.path.join(HERE, "neumf_eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

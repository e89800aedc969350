#!/usr/bin/env python3
"""Generate tests/golden/nmf_eval.npz (CPU, where sklearn and the upstream reference exist; see make_golden.py).

Stored:
  <case>_X, <case>_W0, <case>_H0      the inputs of a solver case, as tests/nmf_ref.py::solver_inputs builds them from the case's seed (X dense), for
                    every case of nmf_ref.SOLVER_CASES and for the early-stop case nmf_ref.EARLY;
  <case>_W, <case>_H, <case>_n_iter   `sklearn.decomposition.NMF(n_components=k, init='custom', solver='cd', max_iter, tol)` fitted on them.
                    For the early-stop case also <case>_ratio: v_i / v_1 of the restatement at the stopping iteration and at the one before it.
  ref_recall, ref_ndcg   [8, 6]: the reference's own `compute_mf_results(train, valid, synthetic, nnmf=True, only_synthetic=True)`
                    (svd_benchmark.py:17-70) on the ML-100k fixture split of tests/svd_eval_ref.py::ml100k_inputs, under np.random.seed(s)
                    for s = 0 .. 7 (rounded to 4 places, as it returns them);
  seed_recall, seed_ndcg [8, 6]: the same chain restated here with sklearn's NMF under the same generator state, UNROUNDED.  The reference
                    reseeds numpy's global generator itself (its hold-out split calls np.random.seed(123)), so the state NMF's randomized SVD
                    draws from does not depend on s: the restatement draws the start for seed s from RandomState(s) instead, which is what the
                    spread over seeds means.  ref_* are asserted equal to the restatement's figures under the reference's own state.
The conditions tests/test_nmf_eval.py puts on the early-stop case are asserted here, so the case is decided by the reference alone.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_nmf_golden.py
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import REFERENCE, load_reference  # noqa: E402
import nmf_ref as nr  # noqa: E402
import svd_eval_ref as sr  # noqa: E402
from sklearn.decomposition import NMF  # noqa: E402
from sklearn.exceptions import ConvergenceWarning  # noqa: E402

warnings.filterwarnings("ignore", category=ConvergenceWarning)


def sklearn_fit(name):
    x, w0, h0, max_iter, tol = nr.solver_inputs(name)
    model = NMF(n_components=w0.shape[1], init="custom", solver="cd", max_iter=max_iter, tol=tol)
    w = model.fit_transform(x, W=w0.copy(), H=h0.copy())
    return w, model.components_.copy(), int(model.n_iter_)


def restated_chain(train, valid, synthetic, random_state):
    """compute_mf_results(nnmf=True, only_synthetic=True) up to the unrounded means, NMF's start drawn from `random_state`."""
    from sdrm_amd import metrics
    from sdrm_amd.pipeline import K_LIST
    test_data, valid_data = metrics.split_train_test_proportion_from_csr_matrix(valid.copy(), batch_size=1000, random_seed=123)
    training = np.concatenate([synthetic.toarray(), test_data.toarray()], axis=0)
    model = NMF(n_components=15, max_iter=50, random_state=random_state)
    recon = model.inverse_transform(model.fit_transform(training))
    masked = metrics.mask_training_examples(sparse_training_set=training, dense_matrix=recon.copy())
    lo = synthetic.shape[0]
    scored = masked[lo:lo + valid_data.shape[0]]
    rec = [np.nanmean(metrics.recall_at_k_batch(scored, valid_data, k=k)) for k in K_LIST]
    ndcg = [np.nanmean(metrics.NDCG_binary_at_k_batch(scored, valid_data, k=k)) for k in K_LIST]
    return np.array(rec), np.array(ndcg)


def main():
    out = {}
    worst = 0.0
    for name in list(nr.SOLVER_CASES) + [nr.EARLY]:
        w, h, n_iter = sklearn_fit(name)
        out[f"{name}_W"], out[f"{name}_H"], out[f"{name}_n_iter"] = w, h, np.asarray(n_iter)
        x, w0, h0, max_iter, tol = nr.solver_inputs(name)
        out[f"{name}_X"], out[f"{name}_W0"], out[f"{name}_H0"] = x.toarray(), w0, h0
        devs = []
        for reverse in (False, True):
            rw, rh, rn, viol = nr.fit(x, w0, h0, max_iter, tol, reverse=reverse)
            assert rn == n_iter, (name, rn, n_iter)
            devs.append(max(nr.normwise(rw, w), nr.normwise(rh, h)))
        worst = max(worst, devs[1])
        print(f"{name}: n_iter {n_iter}, restatement against sklearn {devs[0]:.2e}, with reversed sums {devs[1]:.2e}")
        if name == nr.EARLY:
            _, _, _, viol = nr.fit(x, w0, h0, max_iter, tol)
            ratio = viol / viol[0]
            assert 2 <= n_iter < max_iter, n_iter
            assert ratio[n_iter - 1] * 1.5 <= tol, ratio                      # the stop is at least 1.5x under tol ...
            assert ratio[n_iter - 2] >= 1.5 * tol, ratio                      # ... and the iteration before it at least 1.5x above
            out[f"{name}_ratio"] = ratio[n_iter - 2:n_iter]
    print(f"largest deviation of the reversed restatement from sklearn: {worst:.2e}")

    load_reference()
    if REFERENCE not in sys.path:
        sys.path.insert(0, REFERENCE)
    import svd_benchmark as up  # type: ignore
    train, valid, synthetic = sr.ml100k_inputs()
    dense_synth = synthetic.toarray()
    ref_rec, ref_ndcg, seed_rec, seed_ndcg = [], [], [], []
    for seed in range(8):
        np.random.seed(seed)
        rec, ndcg = up.compute_mf_results(train, valid.copy(), synthetic_data=dense_synth, nnmf=True, only_synthetic=True)
        ref_rec.append(rec)
        ref_ndcg.append(ndcg)
        np.random.seed(seed)
        own = restated_chain(train, valid, synthetic, None)   # the reference's own state: numpy's global generator behind the split
        assert np.array_equal(np.round(own[0], 4), rec) and np.array_equal(np.round(own[1], 4), ndcg), (seed, own, rec, ndcg)
        rec_s, ndcg_s = restated_chain(train, valid, synthetic, np.random.RandomState(seed))
        seed_rec.append(rec_s)
        seed_ndcg.append(ndcg_s)
        print(f"seed {seed}: reference recall {rec}, restated with RandomState({seed}) {np.round(rec_s, 4)}")
    out["ref_recall"], out["ref_ndcg"] = np.stack(ref_rec), np.stack(ref_ndcg)
    out["seed_recall"], out["seed_ndcg"] = np.stack(seed_rec), np.stack(seed_ndcg)
    print("spread of the reference over its 8 calls (recall):", out["ref_recall"].std(axis=0, ddof=1))
    print("mean / std over RandomState(0..7), recall:", out["seed_recall"].mean(axis=0), out["seed_recall"].std(axis=0, ddof=1))
    print("mean / std over RandomState(0..7), ndcg:", out["seed_ndcg"].mean(axis=0), out["seed_ndcg"].std(axis=0, ddof=1))
    np.savez_compressed(os.path.join(HERE, "nmf_eval.npz"), **out)


if __name__ == "__main__":
    main()

"""The callers either side of the denoising path, restated so the end-to-end metric of the reference
(Recall@k / NDCG@k of a downstream SVD recommender trained on the generated data) can be reproduced on
the GPU box, where the reference itself cannot travel.  SURVEY.md §8f ("next" rows).

    load_split / partial_valid      dataloaders.py:82-116  (train_test + the 80 % part of a seeded per-user split of valid)
    batch_feed                      main.py:126-137        (BatchSampler(RandomSampler) index batches -> sparse COO tensors)
    equal_sparsity                  main.py:177-185        (threshold at the data's sparsity quantile)
    equal_sparsity_csr              main.py:177-180, :259-270  (the same as a csr_matrix made on the device, either side)
    compute_mf_results              svd_benchmark.py:17-70 (TruncatedSVD(20, n_iter=100) reconstruction, masked, Recall/NDCG@k)
    compute_mf_results_device       the same evaluator with fit, reconstruction and ranking on the device (opt-in)
    compute_mf_results_resident     ... from a CSR that is already on the device, stacked and transposed there (opt-in)
                                    (all three with `nnmf=True`: svd_benchmark.py:49-50, NMF(15, max_iter=50) in the SVD's place)
    run_experiment                  main.py:143-200        (train -> multi-res + full-res sampling -> evaluate)
"""
from __future__ import annotations

import numpy as np
import torch
from scipy.sparse import csr_matrix, issparse, vstack

from . import metrics
from .mlp_eval import compute_mlp_results_device
from .neumf import compute_neuralcf_results_synthetic

K_LIST = (1, 3, 5, 10, 20, 50)


def csr_from_npz(z, tag):
    shape = tuple(int(v) for v in z[tag + "_shape"])
    return csr_matrix((z[tag + "_data"].astype(np.float64), z[tag + "_indices"].astype(np.int32), z[tag + "_indptr"]), shape=shape)


def load_split(npz_path):
    """(TRAIN_DATA, TRAIN_PARTIAL_VALID_DATA, VALID_DATA) as dataloaders.load_data returns them."""
    z = np.load(npz_path)
    train_test, valid = csr_from_npz(z, "train_test"), csr_from_npz(z, "valid")
    val_train, _ = metrics.split_train_test_proportion_from_csr_matrix(valid, batch_size=1000, random_seed=123, test_prop=0.2)
    return train_test, vstack((train_test, val_train)).tocsr(), valid


def batch_feed(data: csr_matrix, batch_size: int, generator: torch.Generator, device="cuda"):
    """One epoch of the reference's feed: a random permutation cut into index batches (last one short),
    each delivered as a sparse COO float tensor [b, N_ITEMS] twice (data, target)."""
    perm = torch.randperm(data.shape[0], generator=generator).numpy()
    for lo in range(0, len(perm), batch_size):
        coo = data[perm[lo:lo + batch_size]].tocoo()
        x = torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]), coo.data.astype(np.float32), coo.shape).to(device)
        yield x, x


class EpochFeed:
    """Re-iterable like a DataLoader: every `iter()` draws a fresh permutation from the carried generator."""

    def __init__(self, data, batch_size, seed=None, device="cuda"):
        self.data, self.batch_size, self.device = data, batch_size, device
        self.gen = torch.Generator(device="cpu")
        if seed is not None:
            self.gen.manual_seed(seed)

    def __iter__(self):
        return batch_feed(self.data, self.batch_size, self.gen, self.device)


class DeviceFeed:
    """The same epoch feed with the CSR matrix resident on the device: every `iter()` draws the
    permutation the reference's RandomSampler would (torch.randperm on the carried CPU generator) and each batch is
    densified in HBM by `sdrm_csr_rows_to_dense` - what `x.to_dense()` (train_SDRM.py:323) would have produced from the
    host-built COO tensor.  Yields dense tensors (`.to_dense()` of a dense tensor is the tensor itself)."""

    def __init__(self, data, batch_size, engine, seed=None):
        self.engine, self.batch_size, self.n_rows = engine, batch_size, data.shape[0]
        self.csr = engine.csr_to_device(data)
        self.gen = torch.Generator(device="cpu")
        if seed is not None:
            self.gen.manual_seed(seed)

    def __iter__(self):
        perm = torch.randperm(self.n_rows, generator=self.gen).to(self.engine.device)
        for lo in range(0, self.n_rows, self.batch_size):
            x = self.engine.csr_rows_to_dense(self.csr, rows=perm[lo:lo + self.batch_size], check=False)
            yield x, x
        self.engine.feed_status()   # the device-side range checks of the epoch's batches, read once (one sync per epoch)

    def latents(self, engine=None):
        """One epoch of the SAME feed as latents: the permutation draw `iter()` would make, each batch encoded by the frozen
        eval-mode VAE encoder loaded into `engine` (default: the feed's own; `Engine.vae_encoder_load`) straight from the CSR
        rows - `sdrm_vae_encode_csr`, no dense batch - or, where the gather does not pay (`train_SDRM.encode_csr_pays`), densified
        and encoded by `sdrm_vae_encode`.  Yields z [b, latent]."""
        from .train_SDRM import encode_csr_pays
        eng = engine if engine is not None else self.engine
        n_rows, n_items = self.csr[3]
        density = float(self.csr[1].numel()) / (float(n_rows) * float(n_items))
        gather = encode_csr_pays(density, n_items, eng._encoder_dims("DeviceFeed.latents")[1])
        perm = torch.randperm(self.n_rows, generator=self.gen).to(eng.device)
        for lo in range(0, self.n_rows, self.batch_size):
            rows = perm[lo:lo + self.batch_size]
            if gather:
                yield eng.vae_encode_csr(self.csr, rows=rows, check=False)
            else:
                yield eng.vae_encode(eng.csr_rows_to_dense(self.csr, rows=rows, check=False))
        eng.feed_status()


def equal_sparsity(raw, sparsity: float, engine) -> np.ndarray:
    """main.py:177-180, `(raw >= np.quantile(raw.flatten(), SPARSITY)).astype(int)`, on the device
    (`sdrm_equal_sparsity`: radix select of the two order statistics + binarise; csrc/select.h).  `raw` may be a
    device tensor (what `sample_ddpm` returns) or a host array; the 0/1 matrix comes back as the host int array the
    downstream recommenders take."""
    return engine.equal_sparsity(raw, float(sparsity)).cpu().numpy().astype(int)


def equal_sparsity_csr(raw, sparsity: float, engine, side=">=") -> csr_matrix:
    """The same binarisation as a `scipy.sparse.csr_matrix` of ints (sorted indices, shape `raw.shape`) built on the device
    (`sdrm_equal_sparsity_csr_begin` / `_end`; csrc/compact.h): what the consumers of `equal_sparsity` make of its dense result
    (`csr_matrix(...)`, `.tocoo()`, main.py:263-270).  Only indptr and indices cross to the host, no dense matrix exists on either
    side.  `side="<="` with `1 - SPARSITY` is the NeuMF branch's other tail, `(F <= np.quantile(F.flatten(), 1 - SPARSITY))`
    (main.py:260)."""
    indptr, indices, shape = engine.equal_sparsity_csr(raw, float(sparsity), side=side)
    indices = indices.cpu().numpy()
    m = csr_matrix((np.ones(indices.shape[0], dtype=int), indices, indptr.cpu().numpy()), shape=shape)
    m.has_sorted_indices = True
    return m


def compute_mf_results(training_dataset, testing_dataset, synthetic_data, only_synthetic=True, nnmf=False):
    """Recall@k and NDCG@k (k = 1,3,5,10,20,50) of a rank-20 truncated SVD fitted on
    [synthetic | 80 % of each test user's items] and scored on the held-out 20 %.  `synthetic_data` may be a scipy sparse
    matrix (`equal_sparsity_csr`): it is densified here, the fit itself is the dense one either way.  `nnmf=True` fits the
    reference's other factorisation in its place, `NMF(n_components=15, max_iter=50)` (svd_benchmark.py:49-50)."""
    from sklearn import decomposition
    test_data, valid_data = metrics.split_train_test_proportion_from_csr_matrix(testing_dataset, batch_size=1000, random_seed=123)
    if issparse(synthetic_data):
        synthetic_data = synthetic_data.toarray()
    synthetic = np.asarray(synthetic_data)
    head = synthetic if only_synthetic else training_dataset.toarray()
    training = np.concatenate([head, test_data.toarray()], axis=0)
    combined = training if only_synthetic else np.concatenate([training, synthetic], axis=0)
    if nnmf:
        import warnings
        from sklearn.exceptions import ConvergenceWarning
        mf = decomposition.NMF(n_components=15, max_iter=50)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=ConvergenceWarning)   # (svd_benchmark.py:14; 50 iterations do not reach tol)
            recon = mf.inverse_transform(mf.fit_transform(combined))
    else:
        svd = decomposition.TruncatedSVD(n_components=20, n_iter=100)
        recon = svd.inverse_transform(svd.fit_transform(combined))
    masked = metrics.mask_training_examples(sparse_training_set=training, dense_matrix=recon[:training.shape[0]].copy())
    lo = head.shape[0]
    scored = masked[lo:lo + valid_data.shape[0]]
    rec = [np.round(np.nanmean(metrics.recall_at_k_batch(scored, valid_data, k=k)), 4) for k in K_LIST]
    ndcg = [np.round(np.nanmean(metrics.NDCG_binary_at_k_batch(scored, valid_data, k=k)), 4) for k in K_LIST]
    return np.array(rec), np.array(ndcg)


def _device_scores(engine, csr_dev, csc_dev, lo, users, seed, nnmf):
    """The validation users' rows of the reconstruction, float32 [users, n_items] on the device: the rank-20 truncated SVD's, or with
    `nnmf` those of the NMF of 15 components and 50 iterations from its NNDSVDa start (csrc/nmf.h)."""
    if nnmf:
        w, h, _, _ = engine.nmf_fit(csr_dev, csc_dev, n_components=15, max_iter=50, seed=seed)
        return engine.nmf_scores(w, h, row0=lo, b=users)
    components, _ = engine.svd_fit(csr_dev, csc_dev, n_components=20, n_iter=100, seed=seed)
    return engine.svd_scores(csr_dev, components, row0=lo, b=users)


def mf_per_user_device(training_dataset, testing_dataset, synthetic_data, engine, only_synthetic=True, seed=0, nnmf=False):
    """The device evaluator up to the per-user figures: (recall [6, users], ndcg [6, users]) float64 numpy arrays for `K_LIST`, nan for
    a user with nothing held out - what `compute_mf_results_device` averages.  `nnmf=True`: the NMF evaluator in the SVD's place."""
    test_data, valid_data = metrics.split_train_test_proportion_from_csr_matrix(testing_dataset, batch_size=1000, random_seed=123)
    synthetic = synthetic_data.tocsr() if issparse(synthetic_data) else csr_matrix(np.asarray(synthetic_data))
    head = synthetic if only_synthetic else training_dataset.tocsr()
    parts = [head.astype(np.float64), test_data.astype(np.float64)] + ([] if only_synthetic else [synthetic.astype(np.float64)])
    combined = vstack(parts).tocsr()
    combined.eliminate_zeros()   # (`mask_training_examples` masks the NONZERO entries of the stacked rows)
    lo, users = head.shape[0], valid_data.shape[0]
    csr_dev, csc_dev = engine.csr_to_device(combined), engine.csc_to_device(combined)
    scores = _device_scores(engine, csr_dev, csc_dev, lo, users, seed, nnmf)
    # the validation users' stacked training rows as a CSR of their own: indptr holds absolute offsets, so a row range is a slice of it
    seen_dev = (csr_dev[0][lo:lo + users + 1], csr_dev[1], None, (users, combined.shape[1]))
    rec, ndcg = engine.rank_metrics(scores, engine.csr_to_device(valid_data), seen_dev, ks=K_LIST)
    return rec.cpu().numpy(), ndcg.cpu().numpy()


def compute_mf_results_device(training_dataset, testing_dataset, synthetic_data, engine, only_synthetic=True, seed=0, nnmf=False):
    """`compute_mf_results` with the fit, the reconstruction and the ranking on the device (opt-in: `hp["device_svd"]`).  The same
    split and the same rows in the same order, stacked as scipy sparse - no dense matrix exists on the host.  The stacked matrix is
    uploaded once in its CSR and CSC forms; `Engine.svd_fit` runs the rank-20, 100-iteration subspace iteration (csrc/svd_eval.h) from
    a Philox start panel keyed by `seed`, `Engine.svd_scores` reconstructs the validation users' rows only, and `Engine.rank_metrics`
    masks them with their stacked training rows and ranks.  Returns the same `(recall[6], ndcg[6])`, nanmean over the users, rounded
    to 4 places.  `synthetic_data` may be dense 0/1 (`equal_sparsity`) or sparse (`equal_sparsity_csr`).  `nnmf=True` is the
    reference's `nnmf=True` (opt-in: `hp["nmf"]`): `Engine.nmf_fit` and `Engine.nmf_scores` in the place of the SVD's two calls."""
    rec, ndcg = mf_per_user_device(training_dataset, testing_dataset, synthetic_data, engine, only_synthetic=only_synthetic, seed=seed, nnmf=nnmf)
    return (np.array([np.round(np.nanmean(rec[q]), 4) for q in range(len(K_LIST))]),
            np.array([np.round(np.nanmean(ndcg[q]), 4) for q in range(len(K_LIST))]))


def mf_per_user_resident(training_dataset, testing_dataset, synthetic_data, engine, only_synthetic=True, seed=0, nnmf=False):
    """`mf_per_user_device` for synthetic data that is already on the device: `synthetic_data` is a device CSR tuple (what
    `Engine.equal_sparsity_csr` returns, or a `csr_to_device` tuple).  The hold-out split of the validation users stays the host's
    (the reference's draw, a few hundred users) and its two small results are uploaded; the stack [head | test | synthetic?] is made
    by `Engine.csr_vstack` and its CSC form by `Engine.csr_transpose` - the synthetic matrix never visits the host.  The fit, the
    scores and the ranking are `mf_per_user_device`'s calls."""
    test_data, valid_data = metrics.split_train_test_proportion_from_csr_matrix(testing_dataset, batch_size=1000, random_seed=123)

    def upload(m):
        m = m.tocsr().astype(np.float64)
        m.eliminate_zeros()   # (`mask_training_examples` masks the NONZERO entries of the stacked rows)
        return engine.csr_to_device(m)
    head = synthetic_data if only_synthetic else upload(training_dataset)
    parts = [head, upload(test_data)] + ([] if only_synthetic else [synthetic_data])
    csr_dev = engine.csr_vstack(parts, check=False)       # (no synchronise of their own: `svd_fit` below reads the status word that
    csc_dev = engine.csr_transpose(csr_dev, check=False)  #  both calls' range checks raise, and raises for them)
    lo, users = int(head[-1][0]), valid_data.shape[0]
    scores = _device_scores(engine, csr_dev, csc_dev, lo, users, seed, nnmf)
    seen_dev = (csr_dev[0][lo:lo + users + 1], csr_dev[1], None, (users, csr_dev[3][1]))
    rec, ndcg = engine.rank_metrics(scores, engine.csr_to_device(valid_data), seen_dev, ks=K_LIST)
    return rec.cpu().numpy(), ndcg.cpu().numpy()


def compute_mf_results_resident(training_dataset, testing_dataset, synthetic_data, engine, only_synthetic=True, seed=0, nnmf=False):
    """`compute_mf_results_device` from a device CSR tuple (opt-in: `hp["resident_svd"]`): the same `(recall[6], ndcg[6])`, with the
    stacking and the CSR -> CSC conversion on the device (`mf_per_user_resident`)."""
    rec, ndcg = mf_per_user_resident(training_dataset, testing_dataset, synthetic_data, engine, only_synthetic=only_synthetic, seed=seed, nnmf=nnmf)
    return (np.array([np.round(np.nanmean(rec[q]), 4) for q in range(len(K_LIST))]),
            np.array([np.round(np.nanmean(ndcg[q]), 4) for q in range(len(K_LIST))]))


def evaluate_synthetic(train, valid, raw, sparsity, engine, hp, seed):
    """The downstream evaluation of ONE synthetic matrix `raw` (dense scores on the engine's device, binarised here to the training
    data's sparsity): the evaluator `hp` chooses, called as `run_experiment` always called it.  `hp["evaluator"] == "mlp"` is the
    reference's `main.py --model mlp` route (main.py:197-214) without augmentation: `compute_mlp_results_device` on the binarised matrix with the
    train epochs, the per-epoch validation RMSE and the final scores on the device (`hp["mlp_epochs"]`, 200 when absent).
    `hp["evaluator"] == "neumf"` is the `--model neumf` route (main.py:218-283, non-augmented): `neumf.compute_neuralcf_results_synthetic`,
    which takes both tails of `raw` on the device, assembles the training triples there (`Engine.neumf_triples`) and trains and ranks NeuMF
    on the device (`hp["neumf_epochs"]`, 20 when absent; `hp["neumf_eval_recall"]`, True when absent, as main.py:283 calls it;
    `hp["neumf_device_ranking"]`, passed on as `device_ranking` only when the key is present: the ranking problem built and its users selected on
    the device).  Without the
    key: `hp["resident_svd"]`, `hp["device_svd"]`, `hp["sparse_synthetic"]` and `hp["nmf"]` as `run_experiment` documents them."""
    binarise = equal_sparsity_csr if hp.get("sparse_synthetic", False) else equal_sparsity   # opt-in: CSR made on the device
    if hp.get("evaluator") == "mlp":
        return compute_mlp_results_device(binarise(raw, sparsity, engine), valid, engine, device_train=True, seed=seed, epochs=hp.get("mlp_epochs", 200))
    if hp.get("evaluator") == "neumf":
        ranking = {"device_ranking": bool(hp["neumf_device_ranking"])} if "neumf_device_ranking" in hp else {}   # opt-in: csrc/neumf_rank.h
        return compute_neuralcf_results_synthetic(train.shape, valid, raw, sparsity, engine, seed=seed, epochs=hp.get("neumf_epochs", 20),
                                                  eval_recall=hp.get("neumf_eval_recall", True), **ranking)
    if hp.get("evaluator") is not None:
        raise ValueError(f"evaluate_synthetic: hp['evaluator'] = {hp['evaluator']!r}; 'mlp' and 'neumf' are the evaluators the key selects")
    nmf = {"nnmf": True} if hp.get("nmf", False) else {}   # opt-in, the two device routes only: the NMF evaluator in the SVD's place (csrc/nmf.h)
    if hp.get("resident_svd", False):   # opt-in: the CSR made on the device stays there, stacked and transposed on the device (csrc/csr_transpose.h)
        return compute_mf_results_resident(train, valid, engine.equal_sparsity_csr(raw, sparsity), engine, only_synthetic=True, seed=seed, **nmf)
    if hp.get("device_svd", False):   # opt-in: the downstream evaluator on the device (csrc/svd_eval.h)
        return compute_mf_results_device(train, valid, binarise(raw, sparsity, engine), engine, only_synthetic=True, seed=seed, **nmf)
    return compute_mf_results(train, valid, binarise(raw, sparsity, engine), only_synthetic=True)


# the pre-stage's opt-in flags that `hp` may carry, under `train_SDRM`'s keyword names
VAE_FLAGS = ("vae_device_feed", "vae_device_holdout", "vae_sparse_input", "vae_device_latent", "vae_device_decoder", "vae_device_optimizer",
             "vae_device_eval")


def run_experiment(split, hp, seed, vae_dir, verbose=False):
    """One run of main.py's loop body with the MI355X engine; returns {"M": (recall, ndcg), "F": ..., "V": ...}.  `hp` may carry the
    seven flags of the VAE pre-stage under the keys `VAE_FLAGS` (each False when absent): those that are set are handed to `train_SDRM`
    under the same names, and an `hp` without them makes the call it always made.  `hp["device_svd"]` (False when absent) sends the
    three evaluations to `compute_mf_results_device` instead of `compute_mf_results`; nothing of it reaches `train_SDRM`.  `hp["resident_svd"]` (False when absent) binarises with
    `Engine.equal_sparsity_csr` and hands the device tuple to `compute_mf_results_resident`: no host copy of the synthetic matrix.
    `hp["nmf"]` (False when absent) makes those two device routes evaluate with `nnmf=True`, the reference's NMF of 15 components.
    `hp["evaluator"] == "mlp"` sends them to the MLP evaluator on the device instead, `hp["evaluator"] == "neumf"` to NeuMF with its training
    triples assembled on the device (`evaluate_synthetic`, which makes the choice per tag and documents their keys)."""
    from . import train_SDRM as ts
    train, train_partial, valid = split
    n_users, n_items = train.shape
    sparsity = 1 - train.nnz / (n_users * n_items)
    torch.manual_seed(seed)
    np.random.seed(seed)
    from .engine import utility_engine
    dl = DeviceFeed(train_partial, hp["batch"], utility_engine())      # CSR resident in HBM, batches densified there
    net, vae = ts.train_SDRM(dl, N_ITEMS=n_items, VAE_HIDDEN=hp["vae_hidden"], VAE_LATENT=hp["latent"], VAE_BATCH_SIZE=hp["vae_batch"],
                             VAE_LR=hp["vae_lr"], DIFF_LATENT=hp["latent"], N_HIDDEN_MLP_LAYERS=hp["H"], DIFF_LR=hp["lr"],
                             DIFF_TRAINING_EPOCHS=hp["epochs"], TIMESTEPS=hp["T"], noise_divider=hp["nd"], VAE_DIR_PATH=vae_dir,
                             TRAIN_PARTIAL_VALID_DATA=train_partial, VALID_DATA=valid, OPTIMIZATION_OBJECTIVE="Recall@10",
                             verbose=verbose, cache_latents=hp.get("cache_latents", False), engine_encode=hp.get("engine_encode", False),
                             **{flag: True for flag in VAE_FLAGS if hp.get(flag, False)})
    out = {}
    M = ts.sample_ddpm(n_users, net, vae, hp["latent"], hp["nd"], timesteps="random", n_timesteps=hp["T"]).detach()
    F = ts.sample_ddpm(n_users, net, vae, hp["latent"], hp["nd"], n_timesteps=hp["T"]).detach()
    V = vae.sample(n_users)
    for tag, raw in (("M", M), ("F", F), ("V", V)):
        out[tag] = evaluate_synthetic(train, valid, raw, sparsity, net.engine(), hp, seed)
    return out

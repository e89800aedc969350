"""The MLP downstream evaluator (reference: mlp_benchmark.py, a Keras model): the module, the Keras-Adam checker and the driver.

The reference is TensorFlow code and TensorFlow is not part of this project's environment, so this file RESTATES it from the Keras
facts named below; parity with Keras itself has not been run.  The torch loop here is the checker; with `device_train=True` an epoch's
batch loop is ONE `Engine.mlp_train_steps` call (csrc/mlp_train.h), and in `compute_mlp_results_device` the per-epoch validation RMSE
and the final `predict` are `Engine.mlp_eval` calls on device CSR rows (csrc/mlp_eval.h): with both, the module's forward never runs.

The model (`get_model`, :37-62, called with layers=[512, 512, 256, 256]: the Dense loop starts at index 1, so the widths are 512, 256,
256).  The input x is a 0 / 1 row of n_items; `Embedding(num_users, 8)` is indexed BY THE INPUT VALUES, so only its rows 0 and 1 are
ever read, and `Flatten` gives a0[b, 8j + f] = E[x_bj][f].  Then three times Dense(relu) followed by Dropout(0.5), and a Dense of
n_items sigmoid outputs.  The Embedding's `mask_zero=True` changes nothing: Flatten and Dense do not consume the mask.
  * Dropout (keras/src/layers/regularization/dropout.py): in training the kept units are scaled by 1 / (1 - rate); identity otherwise.
  * Loss `binary_crossentropy` (keras/src/losses/losses.py): the mean over the LAST axis, then the mean over the batch - over all
    b n_items elements, for a short last batch of b rows too.  Keras clips the probability to [1e-7, 1 - 1e-7] and takes logs (or,
    depending on the version and backend, recovers the logits from the sigmoid op); HERE the loss is the logits form max(y, 0) - y x +
    log1p(exp(-|y|)).  This is the one chosen deviation of the arithmetic: the two agree until |y| is about 16, where the clip sets in.
  * Optimizer `Adam(learning_rate=1e-3)` (keras/src/optimizers/adam.py, update_step), t = 1, 2, ..:
    alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t); m += (g - m)(1 - beta1); v += (g^2 - v)(1 - beta2); p -= alpha m / (sqrt(v) + eps)
    with betas (0.9, 0.999) and eps = 1e-7 - beside sqrt(v), where torch puts it beside sqrt(v / (1 - beta2^t)).  `KerasAdam` below.
    The embedding's gradient is sparse (IndexedSlices) and Keras updates the indexed rows only: rows 2 .. never move.
  * `fit(validation_split=0.2)` (keras/src/trainers/data_adapters/array_slicing.py, train_validation_split): the LAST n - floor(0.8 n)
    rows are the validation rows, taken before any shuffle; the others are reshuffled every epoch and walked in batches of 16.
  * `RootMeanSquaredError` on the validation rows: sqrt(total squared error / count) over all elements, in inference mode.
  * `EarlyStopping(patience=10, min_delta=0.001, mode='min', restore_best_weights=True)` (keras/src/callbacks/early_stopping.py): an
    epoch improves iff rmse < best - 0.001; the wait counter is reset on an improvement and incremented otherwise; training stops when
    it reaches 10.  The best epoch's weights are restored when training stops early; when all epochs ran, Keras versions differ
    (older ones keep the last epoch's weights) - HERE the best epoch's weights are restored in both endings.
  * Initialisers (keras/src/initializers/random_initializers.py): HeNormal for E - a normal of std sqrt(2 / num_users) truncated at two
    standard deviations (VarianceScaling divides the std by 0.87962566 to make up for the truncation); GlorotUniform for the three Dense
    kernels; `lecun_uniform` for the prediction kernel; zero biases.  Only the distributions are restated: every draw is torch's.
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch
import torch.nn as nn
from scipy.sparse import csr_matrix, issparse, vstack

from . import metrics

K_LIST = (1, 3, 5, 10, 20, 50)
LR, EPOCHS, BATCH, FACTORS, DROPOUT = 1e-3, 200, 16, 8, 0.5      # :27-31
WIDTHS = (512, 256, 256)                                         # :32 through the loop of :50
BETAS, EPS = (0.9, 0.999), 1e-7                                  # keras Adam's defaults
PATIENCE, MIN_DELTA, VALIDATION_SPLIT = 10, 0.001, 0.2           # :96-101, :104
PREDICT_BATCH = 256


class MLP(nn.Module):
    """The reference's model with its parameters in Keras's own layout and order, so that `model.get_weights()` of the reference loads
    as it is (`load_keras_weights`): E [num_users, 8], then the kernels as [in, out] - W1 [8 n_items, 512], W2 [512, 256], W3 [256,
    256], W4 [256, n_items] - each followed by its bias.  W1's row 8j + f is contiguous and item j owns eight adjacent rows."""

    NAMES = ("E", "W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4")

    def __init__(self, num_users, n_items, dropout=DROPOUT):
        super().__init__()
        self.num_users, self.n_items, self.p_drop = int(num_users), int(n_items), float(dropout)
        if self.num_users < 2:
            raise ValueError("MLP: the embedding needs rows 0 and 1 (num_users >= 2)")
        dims = (FACTORS * self.n_items,) + WIDTHS + (self.n_items,)
        self.E = nn.Parameter(torch.empty(self.num_users, FACTORS))
        std = math.sqrt(2.0 / self.num_users) / 0.87962566103423978
        nn.init.trunc_normal_(self.E, mean=0.0, std=std, a=-2.0 * std, b=2.0 * std)
        for l in range(4):
            w = torch.empty(dims[l], dims[l + 1])
            limit = math.sqrt(6.0 / (dims[l] + dims[l + 1])) if l < 3 else math.sqrt(3.0 / dims[l])
            nn.init.uniform_(w, -limit, limit)
            setattr(self, f"W{l + 1}", nn.Parameter(w))
            setattr(self, f"b{l + 1}", nn.Parameter(torch.zeros(dims[l + 1])))

    def engine_weights(self):
        """The nine parameters themselves, in Keras's order (`Engine.MLP_TENSORS`): what `Engine.mlp_train_steps` updates in place."""
        return [getattr(self, n) for n in self.NAMES]

    @torch.no_grad()
    def load_keras_weights(self, arrays):
        """Nine arrays in `get_weights()` order, as they are."""
        arrays = list(arrays)
        if len(arrays) != len(self.NAMES):
            raise ValueError(f"MLP: {len(arrays)} arrays, get_weights() of the reference's model has nine")
        for p, a in zip(self.engine_weights(), arrays):
            a = torch.as_tensor(np.asarray(a))
            if tuple(a.shape) != tuple(p.shape):
                raise ValueError(f"MLP: an array of shape {tuple(a.shape)} where {tuple(p.shape)} is expected")
            p.copy_(a.to(p.dtype))

    def forward(self, x, keep=None):
        """The LOGITS y [b, n_items] of dense 0 / 1 rows x [b, n_items] (the model's output is sigmoid(y): `predict`).  Train mode when the
        module is: the keep decisions of the three dropouts are `keep` [b, 1024] (512 + 256 + 256 columns, non-zero = kept) or, without,
        drawn from torch's generator.  Values outside {0, 1} raise."""
        if x.dim() != 2 or x.shape[1] != self.n_items:
            raise ValueError(f"MLP: the input must be [b, {self.n_items}], got {tuple(x.shape)}")
        if not bool(((x == 0) | (x == 1)).all()):
            raise ValueError("MLP: the input must be 0 / 1 (the reference indexes a two-row embedding with it)")
        h = self.E[x.long()].reshape(x.shape[0], FACTORS * self.n_items)
        if self.training:
            if keep is None:
                keep = torch.rand(x.shape[0], sum(WIDTHS), device=x.device) >= self.p_drop
            elif tuple(keep.shape) != (x.shape[0], sum(WIDTHS)):
                raise ValueError(f"MLP: keep must be [b, {sum(WIDTHS)}], got {tuple(keep.shape)}")
            scale = float(np.float32(1.0 / (1.0 - np.float64(np.float32(self.p_drop)))))
        at = 0
        for l, width in enumerate(WIDTHS):
            h = torch.relu(h @ getattr(self, f"W{l + 1}") + getattr(self, f"b{l + 1}"))
            if self.training:
                h = h * (keep[:, at:at + width] != 0).to(h.dtype) * scale
            at += width
        return h @ self.W4 + self.b4

    @torch.no_grad()
    def predict(self, x):
        """`model.predict`: sigmoid(y) in inference mode, whatever mode the module is in."""
        was = self.training
        self.eval()
        out = torch.sigmoid(self(x))
        self.train(was)
        return out


def bce_from_logits(y, x):
    """`binary_crossentropy` in the logits form, the mean over ALL elements of the batch."""
    return (torch.clamp(y, min=0) - y * x + torch.log1p(torch.exp(-y.abs()))).sum() / y.numel()


class KerasAdam:
    """Keras's Adam over a list of tensors with `.grad` (see the module docstring); the moments are `exp_avg` and `exp_avg_sq`, the step
    count `t`.  A dense update: for the embedding it equals Keras's sparse one as long as the moments of rows 2 .. are zero, which they
    are from a zero start since those rows' gradients are zero."""

    def __init__(self, params, lr=LR, betas=BETAS, eps=EPS):
        self.params = list(params)
        self.lr, self.betas, self.eps, self.t = float(lr), (float(betas[0]), float(betas[1])), float(eps), 0
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    @torch.no_grad()
    def step(self):
        self.t += 1
        b1, b2 = self.betas
        alpha = self.lr * math.sqrt(1.0 - b2 ** self.t) / (1.0 - b1 ** self.t)
        for p, m, v in zip(self.params, self.exp_avg, self.exp_avg_sq):
            if p.grad is None:
                continue
            g = p.grad
            m.add_((g - m) * (1.0 - b1))
            v.add_((g * g - v) * (1.0 - b2))
            p.sub_(alpha * m / (v.sqrt() + self.eps))


class EarlyStop:
    """The bookkeeping of `EarlyStopping(patience, min_delta, mode='min')`: `update(value)` is True iff the epoch improved."""

    def __init__(self, patience=PATIENCE, min_delta=MIN_DELTA):
        self.patience, self.min_delta = int(patience), float(min_delta)
        self.best, self.wait, self.best_epoch, self.epoch = math.inf, 0, None, -1

    def update(self, value):
        self.epoch += 1
        if value < self.best - self.min_delta:
            self.best, self.wait, self.best_epoch = value, 0, self.epoch
            return True
        self.wait += 1
        return False

    @property
    def stop(self):
        return self.wait >= self.patience


def _dense(rows_csr, device, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(rows_csr.toarray(), dtype=np.float32)).to(device=device, dtype=dtype)


def validation_rmse(model, rows_csr, device):
    """`RootMeanSquaredError` of the model in inference mode over all elements of the rows: sqrt(total squared error / count)."""
    total, count = 0.0, 0
    for s in range(0, rows_csr.shape[0], PREDICT_BATCH):
        x = _dense(rows_csr[s:s + PREDICT_BATCH], device)
        total += float(((model.predict(x) - x).double() ** 2).sum().item())
        count += x.numel()
    return math.sqrt(total / count) if count else float("nan")


def _binary_csr(m, name):
    m = (m.tocsr() if issparse(m) else csr_matrix(np.asarray(m))).astype(np.float32)
    m.sum_duplicates()
    m.eliminate_zeros()
    if m.nnz and not np.all(m.data == 1):
        raise ValueError(f"compute_mlp_results: {name} must be 0 / 1")
    m.sort_indices()
    return m


def compute_mlp_results(training_data, validation_data, combine_training=False, engine=None, seed=0, epochs=EPOCHS, device=None, history=None,
                        device_train=False):
    """The reference's driver (mlp_benchmark.py:72-126) over 0 / 1 matrices (scipy sparse or dense): (recall [6], ndcg [6]) for `K_LIST`,
    nanmean over the validation users rounded to 4 places.  As the reference: the model above for n_users = the training rows BEFORE
    `combine_training` appends the 80 % part of the validation users' hold-out split (`batch_size=10, random_seed=123`); the fit, the
    validation split, the RMSE and the early stop as the module docstring restates them; then `predict` on that 80 % part,
    `mask_training_examples`, Recall@k and NDCG@k against the 20 % part.
    The reference's shuffles are Keras's; here every shuffle comes from `numpy.random.default_rng(seed)` (one permutation of the
    floor(0.8 n) train rows per epoch), the initialisation and the torch loop's dropout from torch's GLOBAL generator, seeded with
    `seed` on entry.  The loop runs on `device` (default: the engine's device, the CPU without one).
    `device_train=True` (needs an engine; the model then lives on the engine's device) replaces the batch loop of every epoch by ONE
    `Engine.mlp_train_steps` call on the device CSR of the training rows, the epoch's row order uploaded as int64; Adam's moments are
    nine zero tensors made once, its step count runs on across the epochs, no autograd runs.  The DROPOUT draws are then the engine's
    Philox4x32-10 of (seed, epoch, the row's place in the epoch's order, column), so the trained weights differ from the torch loop's as
    two seeds of it differ.  The per-epoch validation RMSE and the final `predict` stay torch on the engine's device - their device form
    is `compute_mlp_results_device`; with an engine the final ranking is `Engine.rank_metrics` and `feed_status()` is asked once per epoch.
    `history`: a dict that receives 'val_rmse' (per epoch), 'train_loss' (every step's loss), 'best_epoch', 'epochs_run', 'per_user'
    (the final per-user recall / ndcg [6, users]) and 'model' (the module that ranked)."""
    return _mlp_results(training_data, validation_data, combine_training, engine, seed, epochs, device, history, device_train, False)


def compute_mlp_results_device(training_data, validation_data, engine, combine_training=False, seed=0, epochs=EPOCHS, history=None, device_train=True):
    """`compute_mlp_results` with the evaluation half on the device as well (named as `pipeline.compute_mf_results_device` is): the same
    driver, results and `history`, on the engine's device.  The per-epoch RMSE comes from ONE `Engine.mlp_eval(..., row0=n_fit,
    n=n - n_fit, out=False, sse=True)` on the training CSR resident on the device (the train loop's upload, else one upload of its own):
    no dense rows, one scalar read back per epoch - which the early stop needs anyway.  The final scores are one `Engine.mlp_eval` on the
    validation users' 80 % part, uploaded once, ranked by `Engine.rank_metrics` in its device-CSR form.  `device_train` chooses the train
    loop as `compute_mlp_results` does: with True (the default here) `MLP.forward` is never called; with False the torch loop trains and
    the trajectory is that of `compute_mlp_results` from the same seed."""
    if engine is None:
        raise ValueError("compute_mlp_results_device needs an engine (the forward runs on the device CSR; the torch path is compute_mlp_results)")
    return _mlp_results(training_data, validation_data, combine_training, engine, seed, epochs, None, history, device_train, True)


def _mlp_results(training_data, validation_data, combine_training, engine, seed, epochs, device, history, device_train, device_eval):
    """The driver behind `compute_mlp_results` (device_eval False) and `compute_mlp_results_device` (True)."""
    train = _binary_csr(training_data, "training_data")
    valid = _binary_csr(validation_data, "validation_data")
    n_users, n_items = train.shape
    device = torch.device(device) if device is not None else (engine.device if engine is not None else torch.device("cpu"))
    if device_train:
        if engine is None:
            raise ValueError("compute_mlp_results: device_train=True needs an engine (the train step runs on the device; there is no host form)")
        if device != engine.device:
            raise ValueError(f"compute_mlp_results: device_train=True trains on the engine's device {engine.device}, not on {device}")
    valid_train, valid_test = metrics.split_train_test_proportion_from_csr_matrix(csr_matrix(valid), batch_size=10, random_seed=123)
    valid_train, valid_test = _binary_csr(valid_train, "hold-out"), _binary_csr(valid_test, "hold-out")
    if combine_training:
        train = _binary_csr(vstack([train, valid_train]), "training_data")
    n = train.shape[0]
    n_fit = int(math.floor(n * (1.0 - VALIDATION_SPLIT)))
    if n_fit < 1 or n_fit == n:
        raise ValueError(f"compute_mlp_results: {n} training rows leave no train part or no validation part")
    held = train[n_fit:]
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    model = MLP(n_users, n_items, dropout=DROPOUT).to(device)
    if device_train:
        live = [p.data for p in model.engine_weights()]            # the parameters' own storage: the engine updates it in place
        exp_avg, exp_avg_sq = [torch.zeros_like(t) for t in live], [torch.zeros_like(t) for t in live]
    else:
        optimizer = KerasAdam(model.engine_weights(), lr=LR, betas=BETAS, eps=EPS)
    if device_train or device_eval:
        csr_dev = engine.csr_to_device(train)
    stopper = EarlyStop(PATIENCE, MIN_DELTA)
    best_weights, val_rmse, train_loss, steps_done, epochs_run = None, [], [], 0, 0
    for epoch in range(int(epochs)):
        epochs_run += 1
        model.train()
        order = rng.permutation(n_fit)
        if device_train:
            rows = torch.from_numpy(order.astype(np.int64)).to(device)
            losses = engine.mlp_train_steps(live, exp_avg, exp_avg_sq, csr_dev, rows, BATCH, steps_done, lr=LR, betas=BETAS, eps=EPS, p_drop=DROPOUT,
                                            seed=seed, call_id=epoch, check=False)
            steps_done += int(losses.numel())
            train_loss.extend(losses.cpu().tolist())
            engine.feed_status()
        else:
            step_losses = []
            for s in range(0, n_fit, BATCH):
                x = _dense(train[order[s:s + BATCH]], device)
                optimizer.zero_grad()
                loss = bce_from_logits(model(x), x)
                loss.backward()
                optimizer.step()
                step_losses.append(loss.detach())
            train_loss.extend(torch.stack(step_losses).double().cpu().tolist())
        model.eval()
        if device_eval:
            sse = engine.mlp_eval([p.data for p in model.engine_weights()], csr_dev, row0=n_fit, n=n - n_fit, out=False, sse=True, check=False)
            rmse = math.sqrt(float(sse.item()) / ((n - n_fit) * n_items))
            engine.feed_status()
        else:
            rmse = validation_rmse(model, held, device)
        val_rmse.append(rmse)
        if stopper.update(rmse):
            best_weights = copy.deepcopy(model.state_dict())
        if stopper.stop:
            break
    best_epoch = stopper.best_epoch
    if best_weights is not None:
        model.load_state_dict(best_weights)
    else:
        best_epoch = epochs_run - 1          # no epoch improved on +inf (a nan RMSE): the live weights rank
    model.eval()
    if device_eval:
        seen_dev = engine.csr_to_device(valid_train)
        scores = engine.mlp_eval([p.data for p in model.engine_weights()], seen_dev)
        rec, ndcg = engine.rank_metrics(scores, engine.csr_to_device(valid_test), seen_dev, ks=K_LIST)
        rec, ndcg = rec.cpu().numpy(), ndcg.cpu().numpy()
    else:
        scores = torch.cat([model.predict(_dense(valid_train[s:s + PREDICT_BATCH], device)) for s in range(0, valid_train.shape[0], PREDICT_BATCH)])
        if engine is not None:
            rec, ndcg = engine.rank_metrics(scores, valid_test, valid_train, ks=K_LIST)
            rec, ndcg = rec.cpu().numpy(), ndcg.cpu().numpy()
        else:
            masked = metrics.mask_training_examples(sparse_training_set=valid_train, dense_matrix=scores.cpu().numpy().astype(np.float64))
            with np.errstate(invalid="ignore", divide="ignore"):
                rec = np.stack([metrics.recall_at_k_batch(masked, valid_test, k=k) for k in K_LIST])
                ndcg = np.stack([metrics.NDCG_binary_at_k_batch(masked, valid_test, k=k) for k in K_LIST])
    if history is not None:
        history.update(val_rmse=val_rmse, train_loss=train_loss, best_epoch=best_epoch, epochs_run=epochs_run, per_user=(rec, ndcg), model=model)
    with np.errstate(invalid="ignore"):
        return (np.array([np.round(np.nanmean(rec[q]), 4) for q in range(len(K_LIST))]),
                np.array([np.round(np.nanmean(ndcg[q]), 4) for q in range(len(K_LIST))]))

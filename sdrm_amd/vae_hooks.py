"""The PyTorch side of the reference's pipeline that the denoising engine sits between: the MultiVAE++ model, its pre-training
and its checkpoint helpers (/root/reference/train_SDRM.py:66-83, :115-188, :206-268).

NOT part of the hot path and not engine code (SURVEY.md section 2 marks the VAE "HOOK - kept in PyTorch" and its pre-training
out of scope): this module exists so that `sdrm_amd.train_SDRM.train_SDRM()` runs end to end when the caller brings no VAE of its
own, and so that the names the reference's module exports (`VAE`, `train_variational_autoencoder`, `checkpoint`, `resume`) stay
importable from the drop-in module, which re-exports them.  A caller that already has a trained VAE - any object with
`encode(x) -> (z, kl)`, `decode(z)`, `eval()`, `parameters()` and `model_is_trained` - passes it as `variational_ae=` and nothing
in here runs."""
from __future__ import annotations

import os
import time

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import metrics as utilities
from . import _lib
from .engine import SdrmError, utility_engine


def _pruned(msg):
    try:  # the reference signals VAE checkpoint IO failures to Optuna (:72,:83)
        import optuna  # type: ignore
        return optuna.TrialPruned(msg)
    except Exception:
        return RuntimeError(msg)


def checkpoint(model, filename, VAE_DIR_PATH):
    """Save model parameters to file (:75-83)."""
    try:
        torch.save(model.state_dict(), os.path.normpath(os.path.join(VAE_DIR_PATH, filename)))
    except Exception:
        print("Failed to save model parameters to %s" % filename)
        raise _pruned("checkpoint failed")


def resume(model, filename, VAE_DIR_PATH):
    """Load model parameters from file (:66-72)."""
    try:
        model.load_state_dict(torch.load(os.path.normpath(os.path.join(VAE_DIR_PATH, filename))))
    except Exception:
        print("Failed to load model parameters from %s" % filename)
        raise _pruned("resume failed")


class VAE(nn.Module):
    """MultiVAE++ (:206-268), PyTorch: the encode/decode hooks the denoising engine sits between."""

    def __init__(self, input_dim, hidden_dim, latent_dim, p_drop=0.5):
        super().__init__()
        self.latent_dim = latent_dim
        self.encoder = nn.Sequential(nn.Linear(input_dim, hidden_dim), nn.Tanh(), nn.Linear(hidden_dim, 2 * latent_dim))
        self.decoder = nn.Sequential(nn.Linear(latent_dim, hidden_dim), nn.Tanh(), nn.Linear(hidden_dim, input_dim))
        self.dropout = nn.Dropout(p=p_drop)
        self.model_is_trained = False
        self.is_training = 0
        self.weight_decay = 0
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight.data)
                m.bias.data.normal_(0.0, 0.001)

    def encode(self, x):
        h = self.encoder(self.dropout(F.normalize(x, p=2, dim=1)))
        mu, logvar = torch.chunk(h, chunks=2, dim=1)
        kl = -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1))
        eps = torch.randn_like(mu)  # consumed even in eval, like the reference (Q12)
        return mu + self.is_training * eps * torch.exp(0.5 * logvar), kl

    def encode_rows(self, feed, lo, hi, seed, step, latent_seed=None):
        """`encode` in train mode for the rows at places lo .. hi-1 of a `SparseFeed`'s order, without a dense batch: normalise,
        dropout and the first Linear are `sparse_input_linear` (the dropout bits are the engine's Philox draws of (seed, step, feed
        row, column), `self.dropout` draws nothing); the rest of the encoder, the KL and the reparameterisation are `encode`'s.
        With `latent_seed` given that rest is `latent_head` instead - launches of csrc/latent.h, the reparameterisation noise being
        the engine's Philox draw of (latent_seed, step, feed row, column) for the feed rows `feed.order[lo:hi]` (lo .. without an
        order): torch's generator is not consumed."""
        pre = sparse_input_linear(self.encoder[0].weight, self.encoder[0].bias, feed, lo, hi, seed, step, self.dropout.p)
        if latent_seed is not None:
            rows = None if feed.order is None else feed.order[lo:hi]
            return latent_head(pre, self.encoder[2].weight, self.encoder[2].bias, rows, lo, latent_seed, step)
        h = self.encoder[1:](pre)
        mu, logvar = torch.chunk(h, chunks=2, dim=1)
        kl = -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1))
        eps = torch.randn_like(mu)
        return mu + self.is_training * eps * torch.exp(0.5 * logvar), kl

    def decode(self, z):
        return self.decoder(z)

    def decode_nll(self, z, csr_dev, rows=None, row0=0, b=None):
        """`multinomial_nll(self.decode(z), ...)` in train mode without a torch Linear: the decoder, the loss against the rows `rows`
        (or row0 .. row0+b-1) of a `csr_to_device` matrix and the backward of both are `decoder_nll` (csrc/decoder_train.h)."""
        return decoder_nll(z, self.decoder[0].weight, self.decoder[0].bias, self.decoder[2].weight, self.decoder[2].bias, csr_dev,
                           rows=rows, row0=row0, b=b)

    def forward(self, x):
        z, kl = self.encode(x)
        return self.decode(z), kl

    def get_l2_reg(self):
        if self.weight_decay <= 0:
            return torch.zeros((), device=next(self.parameters()).device)
        return self.weight_decay * sum(torch.norm(p, p=2) ** 2 for n, p in self.named_parameters() if n.endswith(".weight"))

    def sample(self, n_samples):
        z = torch.randn(n_samples, self.latent_dim, device=next(self.parameters()).device)
        return self.decode(z).cpu().detach().numpy()


class _MultinomialNLL(torch.autograd.Function):
    """`-mean(sum(log_softmax(logits) * X))` (:141-142) with X given as CSR rows on the device: both directions are launches of
    csrc/nll.h on the utility engine, once-differentiable, nothing is read back (the range checks wait for `feed_status()`)."""

    @staticmethod
    def forward(ctx, logits, csr_dev, rows, row0, b):
        eng = utility_engine(logits.device)
        logits = logits.detach().contiguous()
        rows = None if rows is None else eng._dev(rows, torch.int64)
        loss, lse = eng.multinomial_nll_csr(logits, csr_dev, rows=rows, row0=row0, b=b, check=False)
        ctx.save_for_backward(logits, lse)
        ctx.batch = (eng, csr_dev, rows, row0, b)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        logits, lse = ctx.saved_tensors
        eng, csr_dev, rows, row0, b = ctx.batch
        scale = grad_output.to(dtype=torch.float32).contiguous()   # its device pointer is the kernel's `scale`
        return eng.multinomial_nll_csr_grad(logits, lse, csr_dev, rows=rows, row0=row0, b=b, scale=scale), None, None, None, None


def multinomial_nll(logits, csr_dev, rows=None, row0=0, b=None):
    """The pre-stage's loss term (:141-142) as a 0-dim device tensor with autograd: `logits` [b, n_items] float32 on a ROCm device
    against the rows `rows` (or row0 .. row0+b-1; default all b = logits.shape[0] rows from row0) of a `csr_to_device` matrix.
    Its backward hands `grad_output` to the gradient kernel as a device scalar.  A CSR out of range surfaces at the next
    `utility_engine().feed_status()`."""
    if not logits.is_cuda:
        raise SdrmError("multinomial_nll: the logits must be on a ROCm device (there is no CPU fallback)")
    if rows is None and b is None:
        b = logits.shape[0]
    return _MultinomialNLL.apply(logits, csr_dev, rows, row0, b)


class SparseFeed:
    """One scipy matrix on the device in both forms the train-mode input layer reads: `csr` (`Engine.csr_to_device`, the forward's
    rows) and `csc` (`Engine.csc_to_device`, the weight gradient's columns), plus the epoch's order.  `set_order(order)` stores the
    order (place -> feed row, int64) and its inverse `pos` (feed row -> place, int32) on the device; without one the order is the
    identity and batches are contiguous row ranges."""

    def __init__(self, m, device=None, engine=None):
        self.engine = utility_engine(device) if engine is None else engine
        self.csr = self.engine.csr_to_device(m)
        self.csc = self.engine.csc_to_device(m)
        self.shape = tuple(int(v) for v in m.shape)
        self.order = self.pos = None

    def set_order(self, order):
        order = np.asarray(order, dtype=np.int64)
        n = self.shape[0]
        if order.shape != (n,) or not np.array_equal(np.sort(order), np.arange(n)):
            raise SdrmError(f"SparseFeed.set_order: the order must be a permutation of the feed's {n} rows")
        pos = np.empty(n, dtype=np.int32)
        pos[order] = np.arange(n, dtype=np.int32)
        self.order = torch.from_numpy(order).to(self.engine.device)
        self.pos = torch.from_numpy(pos).to(self.engine.device)


class _SparseInputLinear(torch.autograd.Function):
    """`Linear(n_items, hidden)(dropout(normalize(X)))` for the X whose rows are places lo .. hi-1 of a `SparseFeed`: both
    directions are launches of csrc/input_layer.h, once-differentiable, no dense X and no stored mask."""

    @staticmethod
    def forward(ctx, w1, b1, feed, lo, hi, seed, step, p_drop):
        eng = feed.engine
        rows = None if feed.order is None else feed.order[lo:hi]
        pre, rowscale = eng.vae_input_layer_fwd(w1.detach().contiguous(), b1.detach().contiguous(), feed.csr, rows=rows, row0=lo, b=hi - lo,
                                                seed=seed, step=step, p_drop=p_drop, check=False)
        ctx.save_for_backward(rowscale)
        ctx.batch = (feed, lo, hi, seed, step, p_drop)
        return pre

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dpre):
        (rowscale,) = ctx.saved_tensors
        feed, lo, hi, seed, step, p_drop = ctx.batch
        dpre = dpre.to(dtype=torch.float32).contiguous()
        dw1 = db1 = None
        if ctx.needs_input_grad[0]:
            dw1 = feed.engine.vae_input_layer_wgrad(dpre, rowscale, feed.csc, pos=feed.pos, lo=lo, b=hi - lo, seed=seed, step=step,
                                                    p_drop=p_drop, check=False)
        if ctx.needs_input_grad[1]:
            db1 = dpre.sum(0)
        return dw1, db1, None, None, None, None, None, None


def sparse_input_linear(w1, b1, feed, lo, hi, seed, step, p_drop):
    """The encoder's input layer in train mode (:242-244 up to the first pre-activation) as a device tensor pre [hi - lo, hidden] with
    gradients for w1 [hidden, n_items] and b1 [hidden]: the batch is the rows at places lo .. hi-1 of `feed`'s order (a
    `SparseFeed`).  Dropout keeps entry (feed row R, column c) by the engine's Philox draw of (seed, step, R, c) - not torch's
    generator.  A feed out of range surfaces at the next `feed.engine.feed_status()`."""
    if not w1.is_cuda:
        raise SdrmError("sparse_input_linear: the weights must be on a ROCm device (there is no CPU fallback)")
    if not 0 <= lo < hi <= feed.shape[0]:
        raise SdrmError(f"sparse_input_linear: SDRM_ERR_SHAPE: places {lo} .. {hi} outside the feed's {feed.shape[0]} rows")
    return _SparseInputLinear.apply(w1, b1, feed, int(lo), int(hi), int(seed), int(step), float(p_drop))


class _LatentHead(torch.autograd.Function):
    """`encode`'s tail in train mode - tanh, the second Linear, chunk, the KL, mu + eps * exp(0.5 * logvar) - for a pre-activation
    on the device: both directions are launches of csrc/latent.h on the utility engine, once-differentiable, nothing is read back."""

    @staticmethod
    def forward(ctx, pre, w2, b2, rows, row0, seed, step, eps):
        eng = utility_engine(pre.device)
        w2d = w2.detach().contiguous()
        z, kl, saved = eng.vae_latent_fwd(pre.detach().contiguous(), w2d, b2.detach().contiguous(), rows=rows, row0=row0, seed=seed,
                                          step=step, eps=eps)
        ctx.save_for_backward(w2d, *saved)
        ctx.eng = eng
        ctx.set_materialize_grads(False)   # an unused output's gradient arrives as None and is passed as null
        return z, kl

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gz, gkl):
        w2d, h1, out2, eps = ctx.saved_tensors
        gz = None if gz is None else gz.to(dtype=torch.float32).contiguous()
        gkl = None if gkl is None else gkl.to(dtype=torch.float32).contiguous()   # its device pointer is the kernel's `gkl`
        dpre, dw2, db2 = ctx.eng.vae_latent_bwd((h1, out2, eps), w2d, gz, gkl)
        need = ctx.needs_input_grad
        return dpre if need[0] else None, dw2 if need[1] else None, db2 if need[2] else None, None, None, None, None, None


def latent_head(pre, w2, b2, rows, row0, seed, step, eps=None):
    """The encoder behind its first pre-activation in train mode (:244-250 with is_training == 1) as device tensors (z [b, latent],
    kl 0-dim) with gradients for pre [b, hidden], w2 [2 latent, hidden] and b2 [2 latent].  `eps=None`: the reparameterisation noise
    of (batch row r, column j) is the engine's Philox draw of (seed, step, feed row, j), the feed rows being `rows` (int64 device
    tensor [b]) or row0 .. row0+b-1 - not torch's generator; a float32 device tensor `eps` [b, latent] is used as it is.  The
    backward hands `kl`'s `grad_output` to the kernel as a device scalar; a `None` gradient of either output is passed as null."""
    if not pre.is_cuda:
        raise SdrmError("latent_head: the pre-activation must be on a ROCm device (there is no CPU fallback)")
    return _LatentHead.apply(pre, w2, b2, rows, int(row0), int(seed), int(step), eps)


class _DecoderNLL(torch.autograd.Function):
    """`-mean(sum(log_softmax(decoder(z)) * X))` (:252-254, :141-142) for decoder = Linear -> Tanh -> Linear given as its four tensors
    and X given as CSR rows on the device: both directions are launches of csrc/decoder_train.h on the utility engine,
    once-differentiable, nothing is read back (the range checks wait for `feed_status()`)."""

    @staticmethod
    def forward(ctx, z, w3, b3, w4, b4, csr_dev, rows, row0, b):
        eng = utility_engine(z.device)
        tensors = tuple(t.detach().contiguous() for t in (z, w3, b3, w4, b4))
        rows = None if rows is None else eng._dev(rows, torch.int64)
        loss, saved = eng.vae_decoder_nll_fwd(*tensors, csr_dev, rows=rows, row0=row0, b=b, check=False)
        ctx.save_for_backward(*tensors, *saved)
        ctx.batch = (eng, csr_dev, rows, row0, b)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        z, w3, b3, w4, b4, h3, logits, lse = ctx.saved_tensors
        eng, csr_dev, rows, row0, b = ctx.batch
        scale = grad_output.to(dtype=torch.float32).contiguous()   # its device pointer is the kernel's `scale`
        need = ctx.needs_input_grad
        grads = eng.vae_decoder_nll_bwd((h3, logits, lse), z, w3, b3, w4, b4, csr_dev, rows=rows, row0=row0, b=b, scale=scale, need_dz=need[0])
        return tuple(g if n else None for g, n in zip(grads, need[:5])) + (None, None, None, None)


def decoder_nll(z, w3, b3, w4, b4, csr_dev, rows=None, row0=0, b=None):
    """The decoder and the loss term of the pre-stage's train half (:252-254, :141-142) as a 0-dim device tensor with gradients for z
    [b, latent], w3 [hidden, latent], b3 [hidden], w4 [n_items, hidden] and b4 [n_items] (float32 on a ROCm device), against the rows
    `rows` (or row0 .. row0+b-1; default all b = z.shape[0] rows from row0) of a `csr_to_device` matrix.  No [b, n_items] tensor passes
    through torch's autograd; the backward hands `grad_output` to the gradient kernel as a device scalar and skips the gradient of a z
    that needs none.  A CSR out of range surfaces at the next `utility_engine().feed_status()`."""
    if not z.is_cuda:
        raise SdrmError("decoder_nll: z must be on a ROCm device (there is no CPU fallback)")
    if rows is None and b is None:
        b = z.shape[0]
    return _DecoderNLL.apply(z, w3, b3, w4, b4, csr_dev, rows, int(row0), b)


SPARSE_INPUT_MAX_HIDDEN = 4096   # the widest hidden layer csrc/input_layer.h takes
LATENT_HEAD_MAX_LATENT = 4096    # the widest latent layer csrc/latent.h takes
DECODER_HEAD_MAX_HIDDEN = 4096   # the widest hidden and latent layers csrc/decoder_train.h takes


ADAM_CHUNK = 4096   # elements per work-group of csrc/vae_adam.h: one float64 L2 partial per chunk of every tensor
DIRECT_STEP = True   # train_variational_autoencoder takes `vae_train_step` when all six flags are in effect (False: the autograd path)


class DeviceAdam:
    """`torch.optim.Adam(params, lr, betas, eps)` in its default form with the update of all tensors in ONE launch
    (`Engine.vae_adam_step`, csrc/vae_adam.h), for float32 parameters on a ROCm device.  `weight_decay` is `VAE.weight_decay`, the
    factor of `get_l2_reg`'s `weight_decay * sum ||W||^2` over the `.weight` tensors (:262-268) - NOT torch.optim.Adam's coupled decay
    of every parameter: its gradient 2 weight_decay W is folded into the update of the weights, so autograd differentiates the loss
    without that term, and the term's value comes out of the same launch as float64 partial sums (`l2_partials`, what
    `Engine.vae_loss_slot` adds).  `named_params`: (name, parameter) pairs, e.g. `model.named_parameters()`.  The moments are allocated
    once, zero.  `state_dict()` / `load_state_dict()` speak `torch.optim.Adam`'s layout: a state moves between the two optimizers in
    either direction (torch's own `weight_decay` entry stays 0 there: the L2 term is the loss's, as in the reference)."""

    def __init__(self, named_params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, engine=None):
        named = list(named_params)
        if not named:
            raise SdrmError("DeviceAdam: no parameters")
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.step_count = 0
        self.engine = engine
        self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.l2_coefs = [self.weight_decay if n.endswith(".weight") else 0.0 for n in self.names]
        self.l2_partials = None
        if self.weight_decay > 0:
            chunks = sum(-(-p.numel() // ADAM_CHUNK) for p in self.params)
            self.l2_partials = torch.zeros(chunks, dtype=torch.float64, device=self.params[0].device)
        self._grad_flat = self._grad_views = None

    def zero_grad(self, set_to_none=True):
        """Sets every parameter's `.grad` to None (no launch: `step` reads whole gradients, it accumulates nothing)."""
        for p in self.params:
            p.grad = None

    def grad_buffers(self):
        """One gradient buffer per parameter, of its shape, as views of ONE flat float32 vector allocated at the first call (each view
        on a 64-byte boundary): what `vae_train_step` has the engine's backward calls write through their `out=` arguments."""
        if self._grad_views is None:
            offs, total = [], 0
            for p in self.params:
                offs.append(total)
                total += -(-p.numel() // 16) * 16
            self._grad_flat = torch.zeros(total, dtype=torch.float32, device=self.params[0].device)
            self._grad_views = [self._grad_flat[o:o + p.numel()].view(p.shape) for o, p in zip(offs, self.params)]
        return self._grad_views

    def step(self, grads=None):
        """One update from `grads` (a list, one tensor per parameter; default each parameter's `.grad`).  A missing or non-contiguous
        gradient raises - it is not skipped."""
        if grads is None:
            grads = [p.grad for p in self.params]
        if len(grads) != len(self.params):
            raise SdrmError("DeviceAdam.step: one gradient per parameter")
        for name, g in zip(self.names, grads):
            if g is None or not g.is_contiguous():
                raise SdrmError(f"DeviceAdam.step: the gradient of {name} is {'None' if g is None else 'not contiguous'}")
        if self.engine is None:
            if not self.params[0].is_cuda:
                raise SdrmError("DeviceAdam.step: the parameters must be on a ROCm device (there is no CPU fallback)")
            self.engine = utility_engine(self.params[0].device)
        with torch.no_grad():
            self.engine.vae_adam_step(self.params, grads, self.exp_avg, self.exp_avg_sq, self.step_count + 1, self.lr,
                                      betas=self.betas, eps=self.eps, l2_coefs=self.l2_coefs if self.weight_decay > 0 else None,
                                      l2_partials=self.l2_partials)
        self.step_count += 1

    def state_dict(self):
        """`torch.optim.Adam.state_dict()`'s layout: state[i] = {step, exp_avg, exp_avg_sq} (empty before the first step, like torch's)
        and one param group."""
        group = torch.optim.Adam([torch.zeros(1)], lr=self.lr, betas=self.betas, eps=self.eps).state_dict()["param_groups"][0]
        group["params"] = list(range(len(self.params)))
        state = {}
        if self.step_count > 0:
            state = {i: {"step": torch.tensor(float(self.step_count), dtype=torch.float32), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
                     for i, (m, v) in enumerate(zip(self.exp_avg, self.exp_avg_sq))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise SdrmError("DeviceAdam.load_state_dict: one param group over this optimizer's parameters is expected")
        g = groups[0]
        if g.get("amsgrad") or g.get("maximize") or g.get("weight_decay"):
            raise SdrmError("DeviceAdam.load_state_dict: amsgrad, maximize and torch's coupled weight_decay have no counterpart here")
        state, ids = sd["state"], g["params"]
        steps = {int(float(state[i]["step"])) for i in ids if i in state}
        if len(steps) > 1 or (state and len([i for i in ids if i in state]) != len(ids)):
            raise SdrmError("DeviceAdam.load_state_dict: every parameter must carry a state, all at one step (or none)")
        with torch.no_grad():
            for k, i in enumerate(ids):
                if i in state:
                    self.exp_avg[k].copy_(state[i]["exp_avg"])
                    self.exp_avg_sq[k].copy_(state[i]["exp_avg_sq"])
                else:
                    self.exp_avg[k].zero_()
                    self.exp_avg_sq[k].zero_()
        self.step_count = steps.pop() if steps else 0
        self.lr, self.betas, self.eps = float(g["lr"]), (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"])


def vae_train_step(model, feed, lo, hi, drop_seed, latent_seed, step, anneal, opt, loss_out, slot):
    """One train step of the pre-stage (:139-150) for the rows at places lo .. hi-1 of `feed`'s order (a `SparseFeed` with an order
    set), as a fixed chain of engine calls under `no_grad`: no `autograd.Function`, no `.grad`, no torch arithmetic but the one
    reduction `db1 = dpre.sum(0)`.  The calls, their arguments, seeds and `step` are those the autograd path makes
    (`encode_rows(..., latent_seed=...)` + `decode_nll` + `backward()`), in the order autograd walks them: input layer, latent head,
    decoder and loss forward; decoder backward (null scale: 1), latent backward with gz = dz and gkl = anneal, input-layer weight
    gradient; then `opt.step(grads=...)` (a `DeviceAdam`) on gradients written through `out=` into `opt.grad_buffers()`, and the
    loss `neg_ll + anneal * kl + l2` into `loss_out[slot]` (`Engine.vae_loss_slot`).  `anneal`: a pair (the float, a one-element
    float32 device tensor holding it - a view of the epoch's uploaded values), or the float alone, which is then uploaded here."""
    eng = feed.engine
    if isinstance(anneal, tuple):
        anneal, anneal_dev = anneal
    else:
        anneal_dev = torch.full((1,), float(anneal), dtype=torch.float32, device=eng.device)
    with torch.no_grad():
        w1, b1, w2, b2 = model.encoder[0].weight, model.encoder[0].bias, model.encoder[2].weight, model.encoder[2].bias
        w3, b3, w4, b4 = model.decoder[0].weight, model.decoder[0].bias, model.decoder[2].weight, model.decoder[2].bias
        dw1, db1, dw2, db2, dw3, db3, dw4, db4 = grads = opt.grad_buffers()
        rows = feed.order[lo:hi]
        b, p_drop = hi - lo, model.dropout.p
        pre, rowscale = eng.vae_input_layer_fwd(w1, b1, feed.csr, rows=rows, row0=lo, b=b, seed=drop_seed, step=step, p_drop=p_drop, check=False)
        z, kl, saved_lat = eng.vae_latent_fwd(pre, w2, b2, rows=rows, row0=lo, seed=latent_seed, step=step)
        neg_ll, saved_dec = eng.vae_decoder_nll_fwd(z, w3, b3, w4, b4, feed.csr, rows=rows, check=False)
        dz = torch.empty_like(z)
        eng.vae_decoder_nll_bwd(saved_dec, z, w3, b3, w4, b4, feed.csr, rows=rows, scale=None, need_dz=True, out=(dz, dw3, db3, dw4, db4))
        dpre = torch.empty_like(pre)
        eng.vae_latent_bwd(saved_lat, w2, dz, anneal_dev, out=(dpre, dw2, db2))
        eng.vae_input_layer_wgrad(dpre, rowscale, feed.csc, pos=feed.pos, lo=lo, b=b, seed=drop_seed, step=step, p_drop=p_drop, out=dw1, check=False)
        torch.sum(dpre, 0, out=db1)
        opt.step(grads=grads)
        eng.vae_loss_slot(neg_ll, kl, anneal, loss_out, slot, l2_partials=opt.l2_partials, weight_decay=opt.weight_decay)


EVAL_BATCH = 500                # users per batch of the evaluation half (:166)


def eval_half_supported(model, n_rows, k, batch=EVAL_BATCH):
    """Whether `Engine.vae_eval_holdout` takes this model, `n_rows` users and cut-off `k`: the C library's own host-side argument check
    (`sdrm_debug_vae_eval_args`, which needs no device), so the envelope is stated once, in csrc/sdrm_hip.hip."""
    rc = _lib.load().sdrm_debug_vae_eval_args(int(model.encoder[0].in_features), int(model.encoder[0].out_features), int(model.latent_dim),
                                              int(n_rows), int(batch), int(k), 0)
    return rc == 0


def evaluate_holdout(model, eng, test_csr_dev, seed, draw, early_stop_metric, batch=EVAL_BATCH, device_forward=False):
    """The evaluation half of one pre-stage epoch (:160-177) on the device: the per-user hold-out split of `test_csr_dev` (a
    `csr_to_device` matrix) by `eng.holdout_split(seed=seed, draw=draw)`, then per batch of `batch` users the dense train part
    (`csr_rows_to_dense`), `model(...)` in eval mode under `no_grad`, and Recall@k / NDCG@k of its scores against the held part with
    the train part masked (`rank_metrics`, device form).  Returns the per-user scores as a float64 device tensor [n_rows] - nan for a
    user with fewer than two entries, whom the reference's split drops.  Nothing is read back; a feed out of range surfaces at the
    next `eng.feed_status()`.  The model is left in eval mode with `is_training = 0`.
    `device_forward=True`: the loop over the batches is ONE engine call, `eng.vae_eval_holdout` (csrc/eval_half.h), on the model's live
    weights - no dense batch, no torch `Linear`, no KL and no `randn_like`; its scores differ from the torch forward's by fp32 rounding."""
    k = int(early_stop_metric.split("@")[1])
    which = 0 if "Recall" in early_stop_metric else 1
    n = int(test_csr_dev[3][0])
    model.eval()
    model.is_training = 0
    valid_train, held = eng.holdout_split(test_csr_dev, seed=seed, draw=draw, check=False)
    if device_forward:
        enc0, enc2, dec0, dec2 = model.encoder[0], model.encoder[2], model.decoder[0], model.decoder[2]
        return eng.vae_eval_holdout(enc0.weight, enc0.bias, enc2.weight, enc2.bias, dec0.weight, dec0.bias, dec2.weight, dec2.bias,
                                    valid_train, held, k, which, batch=batch, check=False)
    scores = torch.empty(n, dtype=torch.float64, device=eng.device)
    with torch.no_grad():
        for lo in range(0, n, batch):
            hi = min(lo + batch, n)
            pred, _ = model(eng.csr_rows_to_dense(valid_train, row0=lo, b=hi - lo, check=False))
            scores[lo:hi] = eng.rank_metrics(pred, held, train=valid_train, ks=(k,), row0=lo)[which][0]
    return scores


def train_variational_autoencoder(model, train_data, test_data, epochs, batch_size, lr, early_stop_metric="NDCG@50",
                                  VAE_DIR_PATH="./", verbose=False, device_feed=False, sparse_input=False, device_holdout=False,
                                  device_latent=False, device_decoder=False, device_optimizer=False, device_eval=False):
    """VAE pre-stage (:115-188): multinomial NLL + annealed KL, early stopping on Recall/NDCG@k of a
    per-user hold-out of `test_data`, best epoch restored.  Plain PyTorch (not part of the hot path) - except, with
    `device_feed=True` and the model on a ROCm device, the feed and the loss head: the CSR matrices stay in HBM, every train and
    evaluation batch is densified there (`csr_rows_to_dense`), the NLL term and its gradient are launches of csrc/nll.h
    (`multinomial_nll`), the per-step losses stay on the device until the epoch's one readback, and the range checks of all those
    launches are asked for once per epoch.  The layers, dropout, the reparameterisation draw, KL, L2, autograd through the Linears
    and Adam stay PyTorch.  With the model on the host the keyword is ignored.
    `sparse_input=True` (with `device_feed=True`, the model on a ROCm device and a hidden layer of at most 4096; ignored otherwise)
    also takes the dense batch out of the train half: `model.encode_rows` + `model.decode` in place of `csr_rows_to_dense` +
    `model(X)`, the input layer and its weight gradient being launches of csrc/input_layer.h straight from the feed's CSR rows and
    CSC columns.  Its dropout bits are the engine's Philox draws keyed by a seed and `anneal_count`, not torch's generator, so such a
    run is not bit-comparable with `device_feed=True` alone; and the seed is ONE extra draw from `np.random` (`randint(2**63)`), taken
    before the first epoch's permutation, so numpy's stream is one draw ahead of the other paths'.  The evaluation half is unchanged.
    `device_holdout=True` (with `device_feed=True` and the model on a ROCm device; ignored otherwise) puts the evaluation half on the
    engine (`evaluate_holdout`): `test_data` is uploaded once before the first epoch, epoch e splits it on the device with
    `holdout_split(seed=holdout_seed, draw=e)`, and the epoch's scores come back in the one readback of the losses.  Such a run's
    split is the engine's Philox split (csrc/holdout.h), not numpy's: `holdout_seed` is ONE extra draw from `np.random`
    (`randint(2**63)`, taken before the first permutation, after `sparse_input`'s seed when both are on), numpy's stream no longer
    advances by one `choice` per user per epoch, and the "skipping user" warning is not printed (such users are empty rows whose nan
    score `np.nanmean` ignores, so the same users count).  The run is therefore not bit-comparable with the other paths.
    `device_latent=True` (with `device_feed=True`, `sparse_input=True` in effect, the model on a ROCm device and a latent layer of at
    most 4096; ignored otherwise) also puts everything behind the first pre-activation of the train half's encode on the engine:
    `model.encode_rows(..., latent_seed=...)`, whose tanh, second Linear, KL and reparameterisation are `latent_head` (csrc/latent.h)
    in both directions.  Its reparameterisation noise is the engine's Philox draw keyed by `latent_seed`, `step = int(anneal_count)`
    and the feed row, not `torch.randn_like`: such a run no longer consumes torch's generator in the train half (the evaluation half's
    `encode` still does) and is not bit-comparable with the other paths.  `latent_seed` is ONE extra draw from `np.random`
    (`randint(2**63)`), taken after `sparse_input`'s and `device_holdout`'s seeds and before the first permutation.
    `device_decoder=True` (with `device_feed=True`, the model on a ROCm device and hidden and latent layers of at most 4096; ignored
    otherwise) puts the decoder and the loss term of the train half on the engine: `model.decode_nll(z, csr, rows=...)` in place of
    `model.decode(z)` + `multinomial_nll`, both directions being `decoder_nll` (csrc/decoder_train.h) - no [batch, n_items] tensor
    passes through torch's autograd and, with all five flags on, the train half runs no torch `Linear`.  `z` comes from `encode_rows`
    (with `sparse_input`) or from `model.encode(X)` (dense feed).  The decoder draws nothing: the flag adds no draw from `np.random` or
    torch, and differs from the same run without it by fp32 rounding alone.  The evaluation half, `decode` and `forward` are unchanged.
    `device_optimizer=True` (with `device_feed=True`, the model on a ROCm device and float32 parameters; ignored otherwise) puts the
    optimizer and the loss value on the engine: `DeviceAdam` in place of `torch.optim.Adam` - one launch of csrc/vae_adam.h over the
    eight tensors per step, `zero_grad()` without a launch - autograd differentiates `neg_ll + anneal * kl` only (the gradient of
    `get_l2_reg` is folded into the update), and the step's loss `neg_ll + anneal * kl + l2` goes through `vae_loss_slot` into a
    per-epoch device buffer that the epoch's one readback takes, in place of `losses.append(loss.detach())` + `torch.stack`.  With
    `weight_decay == 0`, the reference's only value, the first step's loss has the bits of the same run without the flag; the updates
    differ from torch's by the rounding of `adam_math`'s hardware `rcp` / `sqrt` (about 1e-7 of an update).  With all six flags in
    effect the step is `vae_train_step`: the same engine calls in the same order with the same arguments, under `no_grad`, without
    an `autograd.Function`, a `.grad` or a torch `Linear` - bit-equal to the autograd path of the same flags (`DIRECT_STEP = False`
    keeps that one) - and the epoch's anneal values are uploaded once per epoch.  The flag adds no draw from `np.random` or torch.
    `device_eval=True` (with `device_feed=True` and `device_holdout=True` in effect, the model on a ROCm device, float32 parameters,
    and what `sdrm_debug_vae_eval_args` accepts - at most 36864 items, hidden and latent layers of at most 4096 and a cut-off
    k <= min(128, n_items) -, asked through `eval_half_supported`; ignored otherwise) puts the
    forward of the evaluation half on the engine too: `evaluate_holdout(..., device_forward=True)`, one `Engine.vae_eval_holdout`
    call per epoch on the live weights (csrc/eval_half.h) in place of `csr_rows_to_dense` + `model(...)` + `rank_metrics` per 500
    users - with it on top of the six flags an epoch runs no torch `Linear` in either half.  The flag adds no draw from `np.random`.
    With it the evaluation half no longer consumes torch's generator: without it `encode` draws a `randn_like` it multiplies by 0.
    Its scores differ from the torch forward's by fp32 rounding, so a near-tie at the cut-off can move a user's metric (and with it
    the epoch's mean and, rarely, the epoch that is restored); the train half is not fed by the evaluation half and does not change."""
    os.makedirs(os.path.normpath(VAE_DIR_PATH), exist_ok=True)
    dev = next(model.parameters()).device
    device_feed = bool(device_feed) and dev.type == "cuda"
    sparse_input = bool(sparse_input) and device_feed and model.encoder[0].out_features <= SPARSE_INPUT_MAX_HIDDEN
    device_holdout = bool(device_holdout) and device_feed
    device_latent = bool(device_latent) and sparse_input and model.latent_dim <= LATENT_HEAD_MAX_LATENT
    device_decoder = (bool(device_decoder) and device_feed and model.decoder[0].out_features <= DECODER_HEAD_MAX_HIDDEN
                      and model.latent_dim <= DECODER_HEAD_MAX_HIDDEN)
    device_optimizer = bool(device_optimizer) and device_feed and all(p.dtype == torch.float32 for p in model.parameters())
    direct_step = DIRECT_STEP and device_optimizer and device_holdout and device_latent and device_decoder
    k = int(early_stop_metric.split("@")[1])
    device_eval = (bool(device_eval) and device_holdout and all(p.dtype == torch.float32 for p in model.parameters())
                   and eval_half_supported(model, test_data.shape[0], k))
    anneal_cap, anneal_count = 0.2, 0.0
    best_metric, best_epoch, stale = -np.inf, 0, 0
    if device_optimizer:
        optimizer = DeviceAdam(model.named_parameters(), lr=lr, weight_decay=getattr(model, "weight_decay", 0.0), engine=utility_engine(dev))
    else:
        optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    start = time.time()
    n = train_data.shape[0]
    if device_feed:
        eng = utility_engine(dev)
        feed = SparseFeed(train_data, engine=eng) if sparse_input else None
        csr = feed.csr if sparse_input else eng.csr_to_device(train_data)
        order = np.arange(n)   # the rows the reference's cumulative train_data = train_data[perm] holds, as an index array
    if sparse_input:
        drop_seed = int(np.random.randint(2 ** 63, dtype=np.int64))
    if device_holdout:
        test_dev = eng.csr_to_device(test_data)
        holdout_seed = int(np.random.randint(2 ** 63, dtype=np.int64))
    latent_seed = int(np.random.randint(2 ** 63, dtype=np.int64)) if device_latent else None
    for epoch in range(epochs):
        losses = []
        model.train()
        model.is_training = 1
        if device_feed:
            order = order[np.random.permutation(n)]
            order_dev = torch.from_numpy(order.astype(np.int64)).to(dev)
            if sparse_input:
                feed.set_order(order)
        else:
            train_data = train_data[np.random.permutation(n)]
        if device_optimizer:
            n_steps = -(-n // batch_size)
            loss_buf = torch.empty(n_steps, dtype=torch.float32, device=dev)   # the epoch's losses, one slot per step
        if direct_step:
            anneal_dev = torch.tensor([min(anneal_cap, 1.0 * (anneal_count + i) / 20_000) for i in range(n_steps)], dtype=torch.float32, device=dev)
        for lo in range(0, n, batch_size):
            hi = min(lo + batch_size, n)
            anneal = min(anneal_cap, 1.0 * anneal_count / 20_000)
            if direct_step:
                slot = lo // batch_size
                vae_train_step(model, feed, lo, hi, drop_seed, latent_seed, int(anneal_count), (anneal, anneal_dev[slot:slot + 1]), optimizer,
                               loss_buf, slot)
                anneal_count += 1
                continue
            if sparse_input:
                X = None
            elif device_feed:
                X = eng.csr_rows_to_dense(csr, rows=order_dev[lo:hi], check=False)
            else:
                X = torch.tensor(train_data[lo:hi].toarray(), dtype=torch.float32, device=dev)
            optimizer.zero_grad()
            if sparse_input:
                if device_latent:
                    z, kl = model.encode_rows(feed, lo, hi, drop_seed, int(anneal_count), latent_seed=latent_seed)
                else:
                    z, kl = model.encode_rows(feed, lo, hi, drop_seed, int(anneal_count))
                out = None if device_decoder else model.decode(z)
            elif device_decoder:
                z, kl = model.encode(X)
            else:
                out, kl = model(X)
            if device_decoder:
                neg_ll = model.decode_nll(z, csr, rows=order_dev[lo:hi])
            elif device_feed:
                neg_ll = multinomial_nll(out, csr, rows=order_dev[lo:hi])
            else:
                neg_ll = -torch.mean(torch.sum(F.log_softmax(out, dim=1) * X, dim=1))
            if device_optimizer:
                (neg_ll + anneal * kl).backward()
                optimizer.step()
                eng.vae_loss_slot(neg_ll.detach(), kl.detach(), anneal, loss_buf, lo // batch_size, l2_partials=optimizer.l2_partials,
                                  weight_decay=optimizer.weight_decay)
                anneal_count += 1
                continue
            loss = neg_ll + anneal * kl + model.get_l2_reg()
            losses.append(loss.detach() if device_feed else loss.item())
            loss.backward()
            optimizer.step()
            anneal_count += 1
        model.eval()
        model.is_training = 0
        scores = []
        if device_holdout:
            scores_dev = evaluate_holdout(model, eng, test_dev, holdout_seed, epoch, early_stop_metric, device_forward=device_eval)
        else:
            valid_train, valid_test = utilities.split_train_test_proportion_from_csr_matrix(test_data, batch_size=1000)
            if device_feed:
                valid_csr = eng.csr_to_device(valid_train)
            with torch.no_grad():
                for lo in range(0, valid_train.shape[0], 500):
                    hi = min(lo + 500, valid_train.shape[0])
                    X = valid_train[lo:hi]
                    if device_feed:
                        pred, _ = model(eng.csr_rows_to_dense(valid_csr, row0=lo, b=hi - lo, check=False))
                    else:
                        pred, _ = model(torch.tensor(X.toarray(), dtype=torch.float32, device=dev))
                    if dev.type == "cuda":
                        # utilities.py:116-171 on the device (sdrm_rank_metrics): the [500, N_ITEMS] scores stay in HBM
                        rec, ndcg = utility_engine(dev).rank_metrics(pred, valid_test[lo:hi], train=X, ks=(k,))
                        scores.append((rec if "Recall" in early_stop_metric else ndcg)[0].cpu().numpy())
                    else:
                        pred = utilities.mask_training_examples(X, pred.cpu().numpy())
                        fn = utilities.recall_at_k_batch if "Recall" in early_stop_metric else utilities.NDCG_binary_at_k_batch
                        scores.append(fn(pred, valid_test[lo:hi], k=k))
        if device_holdout:
            eng.feed_status()
            losses_dev = loss_buf if device_optimizer else torch.stack(losses)
            both = torch.cat([losses_dev.double(), scores_dev]).cpu().numpy()   # one readback: the losses and the scores
            losses, scores = both[:losses_dev.numel()], [both[losses_dev.numel():]]
        elif device_feed:
            eng.feed_status()   # the epoch's one verdict on every row id and column index its launches met
            losses_dev = loss_buf if device_optimizer else torch.stack(losses)
            losses = losses_dev.cpu().numpy().astype(np.float64)   # one readback; the values the .item()s would have been
        avg = np.nanmean(np.concatenate(scores))
        if verbose:
            print(f"Epoch: {epoch}, Loss: {np.round(np.mean(losses), 4)}, {early_stop_metric}: {np.round(avg, 4)}", end="\r")
        if avg > best_metric:
            best_metric, best_epoch, stale = avg, epoch, 0
            checkpoint(model, f"epoch-{epoch}.pth", VAE_DIR_PATH)
        else:
            stale += 1
            if stale > 20:
                if verbose:
                    print(f"MultiVAE++ training complete. Early stopping at epoch {epoch}, "
                          f"Training took {np.round((time.time() - start) / 60, 2)} minutes")
                break
    resume(model, f"epoch-{best_epoch}.pth", VAE_DIR_PATH)
    model.model_is_trained = True
    model.is_training = 0



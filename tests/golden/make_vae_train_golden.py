#!/usr/bin/env python3
"""Generate tests/golden/vae_train_steps.npz from the upstream reference (CPU, where the reference exists; see make_golden.py).

The reference's own `train_variational_autoencoder` on its own `VAE` (train_SDRM.py:115-188, :206-264), fp32, for shape S1 of
tests/vae_step_ref.py: two epochs of three steps, lr 1e-3, `cuda2 = False`, the parameters injected from the shape's tensors.  Its
randoms are replaced by the restated engine draws so that a float64 statement of the step can be held to it:

  * `model.dropout` is a module that in training mode multiplies by `keep_mask(drop_seed, step, rows) * scale(p)`;
  * `torch.randn_like` returns `draw_eps(latent_seed, step, rows)` in training mode (zeros in the evaluation half, which multiplies
    them by `is_training == 0`);
  * `rows` are the feed rows of the current batch, known from the reference's own `np.random.permutation` calls made in training
    mode (recorded and applied cumulatively, as `train_data = train_data[perm]` does) and the count of optimizer steps.

The seeds are the first three draws of `schedule(np_seed)`, taken from `np.random` before the reference runs, so its first epoch is the
replayed schedule's; its evaluation half then draws from `np.random` too (the host split), so the later epochs' rows are stored, not
replayed.  A wrapper round `torch.optim.Adam.step` snapshots the gradients and the parameters after each step, one round
`Tensor.backward` takes the loss.  Stored, float32: seeds and dims, the initial state, and per step the rows, the loss, the eight
gradients and the eight parameters after.  Nothing of the reference's text is stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_vae_train_golden.py
"""
from __future__ import annotations

import io
import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import load_reference  # noqa: E402
import torch  # noqa: E402
import vae_input_layer_ref as vil  # noqa: E402
import vae_latent_ref as vlr  # noqa: E402
import vae_step_ref as vsr  # noqa: E402

SHAPE = "S1"


def save_npz(path, arrays):
    """`np.savez_compressed` with the members' time stamps fixed: two runs give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    ref = load_reference()
    s = vsr.shape_inputs(SHAPE)
    users, items, latent, batch, p = s["users"], s["items"], s["latent"], s["batch"], s["p_drop"]
    m = s["m"]
    np.random.seed(s["np_seed"])
    drop_seed, holdout_seed, latent_seed = (int(np.random.randint(2 ** 63, dtype=np.int64)) for _ in range(3))
    assert (drop_seed, latent_seed) == (s["sched"]["drop_seed"], s["sched"]["latent_seed"])

    torch.manual_seed(0)
    model = ref.VAE(items, s["hidden"], latent, p_drop=p)
    model.cuda2 = False
    assert model.weight_decay == 0 == s["weight_decay"]
    with torch.no_grad():
        for i, ((name, q), t) in enumerate(zip(model.named_parameters(), s["tensors"])):
            assert name == vsr.NAMES[i] and tuple(q.shape) == t.shape, name
            q.copy_(torch.from_numpy(t))
    init = {name: q.detach().numpy().copy() for name, q in model.named_parameters()}

    state = dict(order=np.arange(users), lo=0, count=0)
    steps = []

    def rows_now():
        return state["order"][state["lo"]:state["lo"] + batch]

    class RestatedDropout(torch.nn.Module):
        def forward(self, x):
            if not self.training:
                return x
            rows = rows_now()
            assert x.shape == (len(rows), items)
            keep = vil.keep_mask(drop_seed, state["count"], rows, items, p)
            return x * torch.from_numpy(keep.astype(np.float32) * vil.scale(p))

    model.dropout = RestatedDropout()
    orig_perm, orig_randn_like = np.random.permutation, torch.randn_like
    orig_step, orig_backward = torch.optim.Adam.step, torch.Tensor.backward

    def permutation(n):
        perm = orig_perm(n)
        if model.training:
            assert n == users
            state["order"], state["lo"] = state["order"][perm], 0
        return perm

    def randn_like(t, **kw):
        if not model.training:
            return torch.zeros_like(t)
        rows = rows_now()
        assert t.shape == (len(rows), latent)
        return torch.from_numpy(vlr.draw_eps(latent_seed, state["count"], rows, latent).astype(np.float32))

    def backward(self, *a, **kw):
        steps.append(dict(rows=rows_now().copy(), loss=np.float32(self.item())))
        return orig_backward(self, *a, **kw)

    def adam_step(self, *a, **kw):
        steps[-1]["grads"] = [q.grad.detach().numpy().copy() for q in model.parameters()]
        out = orig_step(self, *a, **kw)
        steps[-1]["after"] = [q.detach().numpy().copy() for q in model.parameters()]
        state["lo"] += batch
        state["count"] += 1
        return out

    np.random.permutation, torch.randn_like = permutation, randn_like
    torch.optim.Adam.step, torch.Tensor.backward = adam_step, backward
    try:
        with tempfile.TemporaryDirectory() as tmp:
            ref.train_variational_autoencoder(model, m, m, vsr.EPOCHS, batch, vsr.LR, early_stop_metric="Recall@10", VAE_DIR_PATH=tmp)
    finally:
        np.random.permutation, torch.randn_like = orig_perm, orig_randn_like
        torch.optim.Adam.step, torch.Tensor.backward = orig_step, orig_backward

    assert len(steps) == len(s["sched"]["steps"]) == 6
    for k in range(3):                                    # the first epoch is the replayed schedule's
        assert np.array_equal(steps[k]["rows"], s["sched"]["steps"][k][0])
    assert all(np.isfinite(st["loss"]) for st in steps)
    out = {"dims": np.asarray([users, items, s["hidden"], latent, batch, vsr.EPOCHS, len(steps)], np.int64),
           "seeds": np.asarray([s["np_seed"], drop_seed, holdout_seed, latent_seed], np.int64),
           "p_drop_lr": np.asarray([p, vsr.LR], np.float64)}
    for i, name in enumerate(vsr.NAMES):
        out[f"init_{i}"] = init[name].astype(np.float32)
    for k, st in enumerate(steps):
        out[f"s{k}_rows"] = st["rows"].astype(np.int64)
        out[f"s{k}_loss"] = np.asarray(st["loss"], np.float32)
        for i in range(len(vsr.NAMES)):
            out[f"s{k}_grad_{i}"] = st["grads"][i].astype(np.float32)
            out[f"s{k}_after_{i}"] = st["after"][i].astype(np.float32)
    path = os.path.join(HERE, "vae_train_steps.npz")
    save_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/neumf_train_<case>.npz, one file per case, from the upstream reference (CPU, where the reference exists; see make_golden.py).

The reference's own `NCF(..., model='NeuMF-end').train()` (neural_cf_benchmark_pt.py:43-144) with `nn.BCEWithLogitsLoss()` and
`optim.Adam(lr=1e-3)` (:167-169), stepped as its batch loop steps it (:195-200), in float32 on the CPU, STEPS consecutive steps per case of
tests/neumf_train_ref.py::CASES.  The dropout masks are made known without touching the reference's arithmetic: torch is seeded, the three
`F.dropout(ones)` of the step are drawn in the module's order and shapes, torch is seeded again the same way and the step runs; the loss
of the float64 restatement under the masks so found must then be the reference's, which is asserted.  Stored per case:
  <case>_seed                     the seed the inputs are rebuilt from: the first from the base seed that meets the kink condition AND at
                                  which the reference's own float32 loss and gradients are within the fp32 bar 1e-4 of the float64
                                  restatement (with N(0, 0.5^2) weights a batch of ONE pair can have a saturated logit, where
                                  float32's sigmoid(y) - 1 keeps two digits: such a draw measures nothing);
  <case>_keep                     the masks of every triple the steps use, bit-packed [n or steps, 14F / 8];
  <case>_dev                      [steps, 3] normwise deviation of the reference's float32 pre-activations from the float64 ones;
  <case>_s<k>_p / _m / _v / _g    per step k the parameters, exp_avg, exp_avg_sq BEFORE the step and its gradients, each the twelve tensors
                                  flattened one behind the other (`neumf_ref.NAMES` order); _m and _v of step 0 are zero and not stored;
  <case>_s<k>_loss                the reference's loss of the step;
  <case>_final_p                  the parameters after the last step.
The other inputs are not stored.  The conditions tests/test_neumf_train.py puts on the cases are asserted here as well.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_neumf_train_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pandas as pd  # noqa: F401  (before load_reference() stubs `bottleneck`: pandas looks for the real one when it is imported)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import load_reference  # noqa: E402
import torch  # noqa: E402
import neumf_train_ref as tr  # noqa: E402

MAX_TRIES = 64
FP32_BAR = 1e-4   # the project's fp32 bar, which tests/test_neumf_train.py holds the reference's own float32 results to


def flat(tensors):
    return np.concatenate([np.asarray(t, dtype=np.float32).ravel() for t in tensors])


def draw_masks(torch_seed, b, F):
    """uint8 [b, 14F]: what the three Dropout modules of the tower draw for a batch of b right after torch.manual_seed(torch_seed)."""
    torch.manual_seed(torch_seed)
    parts = [torch.nn.functional.dropout(torch.ones(b, width), p=tr.P_DROP, training=True) for width in (8 * F, 4 * F, 2 * F)]
    return (torch.cat(parts, dim=1) != 0).numpy().astype(np.uint8)


def run_case(up, name, seed):
    """The case at `seed`: the fixture entries, or the reason (a string) why the seed is passed over."""
    F, n_users, n_items, n, batches, _ = tr.CASES[name]
    w, tri = tr.case_inputs(name, seed)
    model = up.NCF(n_users, n_items, F, 3, tr.P_DROP, "NeuMF-end").train()
    assert list(model.state_dict()) == list(tr.NAMES)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    loss_function = torch.nn.BCEWithLogitsLoss()
    optimizer = torch.optim.Adam(model.parameters(), lr=tr.LR)
    params = list(model.parameters())
    pre = {}
    for idx, layer in ((0, 1), (1, 4), (2, 7)):
        model.MLP_layers[layer].register_forward_hook(lambda m, i, o, idx=idx: pre.__setitem__(idx, o.detach().numpy().copy()))
    out = {f"{name}_seed": np.asarray(seed)}
    distinct = len(set(batches)) == len(batches)
    keep_all = np.zeros((n if distinct else len(batches), 14 * F), dtype=np.uint8)
    devs = []
    for k, (lo, hi) in enumerate(batches):
        x = torch.from_numpy(tri[lo:hi].copy())
        torch_seed = 1000 * seed + k
        keep = draw_masks(torch_seed, hi - lo, F)
        if distinct:
            keep_all[lo:hi] = keep
        else:
            keep_all[k:k + 1] = keep
        before = {kname: v.detach().numpy().copy() for kname, v in model.state_dict().items()}
        out[f"{name}_s{k}_p"] = flat(before.values())
        if k > 0:
            out[f"{name}_s{k}_m"] = flat([optimizer.state[p]["exp_avg"].numpy() for p in params])
            out[f"{name}_s{k}_v"] = flat([optimizer.state[p]["exp_avg_sq"].numpy() for p in params])
        torch.manual_seed(torch_seed)
        model.zero_grad()
        prediction = model(x[:, 0], x[:, 1])
        loss = loss_function(prediction, x[:, 2].float())
        loss.backward()
        ref64 = tr.step64(before, tri[lo:hi], keep)
        dev = [tr.normwise(pre[l], ref64["z"][l]) for l in range(3)]
        # masks that were not the reference's would move the loss by a whole term, not by a rounding
        assert abs(ref64["loss"] - loss.item()) <= 1e-3 * max(1.0, abs(ref64["loss"])), ("the stored masks are not the reference's", name, k, ref64["loss"], loss.item())
        if any(tr.kink_exceptions(ref64["z"], dev)):
            return "a pre-activation inside the gap"
        if abs(ref64["loss"] - loss.item()) > FP32_BAR * abs(ref64["loss"]):
            return "the reference's float32 loss misses the fp32 bar (a saturated logit)"
        devs.append(dev)
        grads = [p.grad.numpy().copy() for p in params]
        for gname, g in zip(tr.NAMES, grads):
            d = tr.normwise(g, ref64["grads"][gname])
            assert d > 0, (name, k, gname)
            if d > FP32_BAR:
                return f"the reference's float32 gradient of {gname} misses the fp32 bar (sigmoid(y) - 1 cancels at a saturated logit)"
        out[f"{name}_s{k}_g"] = flat(grads)
        out[f"{name}_s{k}_loss"] = np.asarray(loss.item(), dtype=np.float32)
        optimizer.step()
    out[f"{name}_final_p"] = flat([v.detach().numpy() for v in model.state_dict().values()])
    out[f"{name}_keep"] = np.packbits(keep_all, axis=1)
    out[f"{name}_dev"] = np.asarray(devs, dtype=np.float64)
    if name == "f8":
        assert all(tr.f8_conditions(tri, batches, n_users)), tr.f8_conditions(tri, batches, n_users)
    print(name, "seed", seed, "fp32 deviation of the pre-activations per step and layer", np.asarray(devs))
    return out


def main():
    load_reference()
    import neural_cf_benchmark_pt as up  # type: ignore

    for name, case in tr.CASES.items():
        base = case[-1]
        for seed in range(base, base + MAX_TRIES):
            got = run_case(up, name, seed)
            if not isinstance(got, str):
                break
            print(name, "seed", seed, "passed over:", got)
        else:
            raise SystemExit(f"{name}: no seed in {base} .. {base + MAX_TRIES - 1} meets the conditions")
        path = os.path.join(HERE, f"neumf_train_{name}.npz")   # a file per case: together they would pass the size limit of a committed file
        np.savez_compressed(path, **got)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

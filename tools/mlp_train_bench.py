#!/usr/bin/env python3
"""One train epoch of the MLP evaluator, two ways, at three shapes (the reference's widths 512 / 256 / 256, batches of 16; rows x items):

  ML-100k fixture   tests/golden/ml100k.npz's train rows, 843 x 1008 as they are
  ML-1M shape       6040 x 3706, 4.5 % of the entries set
  ADM shape         5541 x 3568, 0.35 %

An epoch walks the first floor(0.8 rows) rows in a shuffled order, as `mlp_eval.compute_mlp_results` does.  Timed, each REPS times with the
spread shown (host clock around work that ends in a device synchronise):

  device   ONE `Engine.mlp_train_steps` call over the epoch's row order (csrc/mlp_train.h), weights and moments carried on from call to call;
  torch    the driver's own loop on the same GPU - the checker, the only reference that can run: per batch the rows densified and uploaded,
           the module's forward, the loss, `backward`, `KerasAdam.step` (mlp_eval.py's loop without `device_train`).

Then, in a window of its own with two events around every launch (shares of the step, not durations to quote), the split of a device step
between its forward, the W1 pass and the rest of the backward; the launches per step from the handle's launch counter; the bytes a step
has to move, computed from the shapes (W1, its two moments and the three small kernels with theirs read and written once, the kernels
read once more by the input gradients and the forward, the gather of the batch's entries, the partial B_f written and read), and the
share of 6.3 TB/s that is over the step's time - and over the W1 pass's time under the profile for the pass's own bytes.
`--out FILE` appends the table to FILE (profiles/mlp_train_bench.txt is such a file)."""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch
from scipy.sparse import csr_matrix

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from sdrm_amd import mlp_eval  # noqa: E402
from sdrm_amd.engine import utility_engine  # noqa: E402

BATCH = mlp_eval.BATCH
H1, H2, H3 = mlp_eval.WIDTHS
SHAPES = {"ML-100k fixture": None, "ML-1M shape": (6040, 3706, 0.045), "ADM shape": (5541, 3568, 0.0035)}
HBM = 6.3e12
REPS = {"device": 5, "torch": 3}
W1_ITEMS = 16   # csrc/mlp_train.h: MLP_W1_ITEMS


def matrix(name, seed=0):
    if SHAPES[name] is None:
        z = np.load(os.path.join(REPO, "tests", "golden", "ml100k.npz"))
        m = csr_matrix((np.ones(z["train_test_indices"].shape[0], dtype=np.float32), z["train_test_indices"].astype(np.int32),
                        z["train_test_indptr"].astype(np.int64)), shape=tuple(int(v) for v in z["train_test_shape"]))
    else:
        rows, items, density = SHAPES[name]
        rng = np.random.default_rng(seed)
        m = csr_matrix((rng.random((rows, items)) < density).astype(np.float32))
    m.sum_duplicates()
    m.data[:] = 1.0
    m.sort_indices()
    return m


def step_bytes(n_items, entries_per_step):
    """Bytes one step has to move, from the shapes."""
    w1 = 8 * n_items * H1 * 4
    small = (H1 * H2 + H2 * H3 + H3 * n_items) * 4
    parts = -(-n_items // W1_ITEMS) * 8 * H1 * 8
    return dict(w1_pass=6 * w1 + parts, gather=entries_per_step * 8 * H1 * 4, small=6 * small + 2 * small, bsum=parts)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(ms):
    return f"{np.median(ms):.1f} ({min(ms):.1f} .. {max(ms):.1f})"


def torch_epoch(model, optimizer, train, order):
    for s in range(0, order.shape[0], BATCH):
        x = mlp_eval._dense(train[order[s:s + BATCH]], "cuda")
        optimizer.zero_grad()
        loss = mlp_eval.bce_from_logits(model(x), x)
        loss.backward()
        optimizer.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mlp_train_bench needs the GPU"
    eng = utility_engine()
    lines = [f"{'one epoch (512 / 256 / 256, batch 16)':<40}{'rows':>6}{'items':>7}{'steps':>7}{'device ms: median (min .. max)':>34}{'us/step':>9}"
             f"{'torch ms: median (min .. max)':>34}{'us/step':>9}{'torch / device':>16}{'beyond the spread':>19}"]
    notes = []
    for name in args.shapes:
        train = matrix(name)
        n_rows, n_items = train.shape
        n_fit = int(math.floor(0.8 * n_rows))
        steps = -(-n_fit // BATCH)
        rng = np.random.default_rng(1)
        torch.manual_seed(0)
        model = mlp_eval.MLP(n_rows, n_items).cuda().train()
        live = [p.data for p in model.engine_weights()]
        m, v = [torch.zeros_like(t) for t in live], [torch.zeros_like(t) for t in live]
        csr_dev = eng.csr_to_device(train)
        state = {"step0": 0, "call": 0}

        def device_epoch():
            rows = torch.from_numpy(rng.permutation(n_fit).astype(np.int64)).cuda()
            eng.mlp_train_steps(live, m, v, csr_dev, rows, BATCH, state["step0"], seed=0, call_id=state["call"], check=False)
            state["step0"] += steps
            state["call"] += 1

        host_ms(device_epoch)                                          # warm-up: code objects, scratch
        n0 = eng.launch_count()
        d_ms = [host_ms(device_epoch) for _ in range(REPS["device"])]
        per_step = (eng.launch_count() - n0) / (REPS["device"] * steps)
        eng.feed_status()
        # the step's split, in a window of its own: the first 100 steps
        n_prof = min(steps, 100)
        rows = torch.from_numpy(rng.permutation(n_fit)[:n_prof * BATCH].astype(np.int64)).cuda()
        n_prof = -(-rows.numel() // BATCH)
        eng.profile_begin(capacity=4096)
        eng.mlp_train_steps(live, m, v, csr_dev, rows, BATCH, state["step0"], seed=0, call_id=999, check=False)
        torch.cuda.synchronize()
        prof = {k: val for k, val in eng.profile_end().items() if k.startswith("mlp train step")}
        total = sum(val[0] for val in prof.values())
        w1_ms, w1_n, _ = next(val for k, val in prof.items() if "k_mlp_w1" in k)
        by = step_bytes(n_items, train[:n_fit].nnz / n_fit * BATCH)
        step_us = np.median(d_ms) / steps * 1e3
        w1_us = w1_ms / w1_n * 1e3
        notes.append(f"{name:<18}launches per step {per_step:.2f} (15 a step and 2 a call); bytes a step must move {sum(by.values()) / 1e6:.1f} MB (W1 pass "
                     f"{by['w1_pass'] / 1e6:.1f}, gather {by['gather'] / 1e6:.1f}, small layers {by['small'] / 1e6:.1f}, B_f partials read {by['bsum'] / 1e6:.1f}) = "
                     f"{sum(by.values()) / (step_us * 1e-6) / HBM:.1%} of 6.3 TB/s at {step_us:.1f} us a step; shares of the step under the profile: "
                     + ", ".join(f"{k.split(':')[1].split()[0]}.. {val[0] / total:.0%}" for k, val in prof.items())
                     + f"; k_mlp_w1 {w1_us:.1f} us per launch under the profile = {by['w1_pass'] / (w1_us * 1e-6) / HBM:.1%} of 6.3 TB/s for its own bytes")
        # the torch loop, a fresh model and optimizer
        torch.manual_seed(0)
        tmodel = mlp_eval.MLP(n_rows, n_items).cuda().train()
        opt = mlp_eval.KerasAdam(tmodel.engine_weights())
        torch_epoch(tmodel, opt, train, rng.permutation(n_fit)[:5 * BATCH])   # warm-up
        t_ms = [host_ms(lambda: torch_epoch(tmodel, opt, train, rng.permutation(n_fit))) for _ in range(REPS["torch"])]
        beyond = min(t_ms) - max(d_ms) > (max(t_ms) - min(t_ms))
        lines.append(f"{name:<40}{n_rows:>6}{n_items:>7}{steps:>7}{spread(d_ms):>34}{step_us:>9.1f}{spread(t_ms):>34}"
                     f"{np.median(t_ms) / steps * 1e3:>9.1f}{np.median(t_ms) / np.median(d_ms):>15.1f}x{'yes' if beyond else 'NO':>19}")
        print(lines[-1], flush=True)
        print(notes[-1], flush=True)
        del model, tmodel, opt, live, m, v
        torch.cuda.empty_cache()
    text = "\n".join(lines + [""] + notes) + "\n\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()

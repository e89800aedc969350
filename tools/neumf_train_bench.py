#!/usr/bin/env python3
"""One NeuMF train epoch, two ways, at three shapes (F = 8, batches of 256, the reference's; users x items, share of the pairs in training):

  ML-100k split   943 x 1008, 6 %
  ML-1M shape     6040 x 3706, 4 %
  ADM shape       5541 x 3568, 0.35 %

An epoch's triples are drawn as `neumf.compute_neuralcf_results` draws them (80 % of the training triples, as many label-0 rows again as
there are label-1 rows, shuffled).  Timed, each REPS times with the spread shown (host clock around work that ends in a device synchronise):

  device   ONE `Engine.neumf_train_steps` call over the epoch's array (csrc/neumf_train.h), moments and weights carried on from call to call;
  torch    the driver's own loop on the same GPU: per batch `torch.as_tensor(...)`, `zero_grad`, forward, BCE-with-logits, `backward`,
           `optim.Adam.step` (neumf.py's loop without `device_train`, which is the loop of the parent commit).

Then, in a window of its own with two events around every launch (shares of the step, not durations to quote), the split of a device step
between its four launches, the launches per step from the handle's launch counter, and for k_nt_pairs the flops the algorithm needs per pair
(forward and input gradients of the tower, 2 x 2 x 42 F^2, and the predict layer) over its time as a share of the fp32 vector peak
(157.3 TFLOP/s).  `--out FILE` appends the table to FILE (profiles/neumf_train_bench.txt is such a file)."""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrm_amd import neumf  # noqa: E402
from sdrm_amd.engine import utility_engine  # noqa: E402

F, BATCH = 8, 256
SHAPES = {"ML-100k split": (943, 1008, 0.06), "ML-1M shape": (6040, 3706, 0.04), "ADM shape": (5541, 3568, 0.0035)}
PEAK_FLOPS = 157.3e12
FLOPS_PER_PAIR = 2 * (2 * 42 * F * F + 4 * F)
REPS = {"device": 7, "torch": 3}


def epoch_triples(name, seed=0):
    n_users, n_items, density = SHAPES[name]
    rng = np.random.default_rng(seed)
    n = int(density * n_users * n_items)
    flat = rng.choice(n_users * n_items, size=n, replace=False)
    training = np.stack([flat // n_items, flat % n_items, rng.integers(0, 2, n)], axis=1).astype(np.int64)
    n_hold = int(math.ceil(0.2 * n))
    part = training[rng.permutation(n)[n_hold:]]
    negatives = part[part[:, 2] == 0]
    part = np.concatenate([part, negatives[rng.integers(0, negatives.shape[0], size=int((part[:, 2] == 1).sum()))]])
    return n_users, n_items, part[rng.permutation(part.shape[0])]


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(ms):
    return f"{np.median(ms):.1f} ({min(ms):.1f} .. {max(ms):.1f})"


def torch_epoch(model, optimizer, part):
    for s in range(0, part.shape[0], BATCH):
        x = torch.as_tensor(part[s:s + BATCH], dtype=torch.int32, device="cuda")
        model.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy_with_logits(model(x[:, 0], x[:, 1]), x[:, 2].float())
        loss.backward()
        optimizer.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "neumf_train_bench needs the GPU"
    eng = utility_engine()
    lines = [f"{'one epoch (F = 8, batch 256)':<30}{'triples':>9}{'steps':>7}{'device ms: median (min .. max)':>34}{'us/step':>9}"
             f"{'torch ms: median (min .. max)':>34}{'us/step':>9}{'torch / device':>16}{'beyond the spread':>19}"]
    shares = []
    for name in args.shapes:
        n_users, n_items, part = epoch_triples(name)
        steps = -(-part.shape[0] // BATCH)
        torch.manual_seed(0)
        model = neumf.NCF(n_users, n_items, factor=F).cuda().train()
        live = model.engine_weights()
        m, v = [torch.zeros_like(t) for t in live], [torch.zeros_like(t) for t in live]
        tri = torch.from_numpy(part.astype(np.int32)).cuda()
        state = {"step0": 0, "call": 0}

        def device_epoch():
            eng.neumf_train_steps(live, m, v, tri, BATCH, state["step0"], seed=0, call_id=state["call"], check=False)
            state["step0"] += steps
            state["call"] += 1

        host_ms(device_epoch)                                          # warm-up: code objects, scratch
        n0 = eng.launch_count()
        d_ms = [host_ms(device_epoch) for _ in range(REPS["device"])]
        per_step = (eng.launch_count() - n0) / (REPS["device"] * steps)
        eng.feed_status()
        # the step's split, in a window of its own: the first 200 steps
        eng.profile_begin(capacity=4096)
        eng.neumf_train_steps(live, m, v, tri[:200 * BATCH], BATCH, state["step0"], seed=0, call_id=99, check=False)
        torch.cuda.synchronize()
        prof = {k: val for k, val in eng.profile_end().items() if k.startswith("neumf train step")}
        total = sum(val[0] for val in prof.values())
        pairs_ms, pairs_n, pairs_fl = next(val for k, val in prof.items() if "k_nt_pairs" in k)
        shares.append(f"{name:<16}launches per step {per_step:.2f}; shares of the step " + ", ".join(f"{k.split(':')[1].split()[0]} {val[0] / total:.0%}" for k, val in prof.items())
                      + f"; k_nt_pairs {pairs_ms / pairs_n * 1e3:.1f} us per launch under the profile, {pairs_fl / (pairs_ms * 1e-3) / 1e12:.2f} TFLOP/s = "
                      f"{pairs_fl / (pairs_ms * 1e-3) / PEAK_FLOPS:.2%} of the fp32 vector peak ({FLOPS_PER_PAIR} flops a pair)")
        # the torch loop, a fresh model and optimizer
        torch.manual_seed(0)
        tmodel = neumf.NCF(n_users, n_items, factor=F).cuda().train()
        opt = torch.optim.Adam(tmodel.parameters(), lr=neumf.LR)
        torch_epoch(tmodel, opt, part[:20 * BATCH])                     # warm-up
        t_ms = [host_ms(lambda: torch_epoch(tmodel, opt, part)) for _ in range(REPS["torch"])]
        beyond = min(t_ms) - max(d_ms) > (max(t_ms) - min(t_ms))
        lines.append(f"{name:<30}{part.shape[0]:>9}{steps:>7}{spread(d_ms):>34}{np.median(d_ms) / steps * 1e3:>9.1f}{spread(t_ms):>34}"
                     f"{np.median(t_ms) / steps * 1e3:>9.1f}{np.median(t_ms) / np.median(d_ms):>15.1f}x{'yes' if beyond else 'NO':>19}")
        print(lines[-1], flush=True)
        print(shares[-1], flush=True)
    text = "\n".join(lines + [""] + shares) + "\n\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()

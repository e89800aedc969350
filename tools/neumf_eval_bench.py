#!/usr/bin/env python3
"""The NeuMF evaluator's evaluation half, three ways, at three shapes (validation users x training items; F = 8, the reference's):

  ML-100k split   95 x 1008    (943 users in all, 6 % of the pairs in training)
  ML-1M shape     1208 x 3706  (6040 users, 4 %)
  ADM shape       554 x 3568   (5541 users, 0.35 %)

  --part kernels  `Engine.neumf_scores` alone (sdrm_neumf_scores: k_neumf_stage + k_neumf_scores), device events around REPS calls after a
                  warm-up; the split between the two kernels from the engine's event profile (two events around every launch: shares, not
                  durations); the all-pairs launch as a fraction of the fp32 vector peak (157.3 TFLOP/s; the flops the algorithm needs per
                  pair behind the staging, 20 F^2 + 13 F) and of the store bandwidth (4 bytes per pair over 6.29 TB/s measured copy rate)
  --part torch    the same matrix from `neumf.NCF` in eval mode on the same GPU in the reference's batches of 10000 pairs (forward only and
                  one concatenation - without the reference's per-batch `.cpu().numpy().flatten().tolist()`), device events
  --part full     one whole evaluation: `neumf.rank_all_items(model, training, validation, users, engine)` end to end (numpy compaction,
                  uploads, two launches, ranking, read-back) against the reference's procedure restated with pandas (forward on the GPU in
                  batches of 10000 moved to a Python list, two left merges, two CSR matrices through dicts, densified, ranked at six k);
                  host clock around work that ends in a device synchronise.  Skipped with a note where pandas does not import.

Every part is one process; run them chained, each under its own time limit, so that nothing starts on the GPU after a part that failed:

    timeout -k 10 240 python tools/neumf_eval_bench.py --part kernels --out F && \
    timeout -k 10 240 python tools/neumf_eval_bench.py --part torch --out F && \
    timeout -k 10 400 python tools/neumf_eval_bench.py --part full --out F

`--out FILE` appends the part's table to FILE (profiles/neumf_eval_bench.txt is such a file)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrm_amd import neumf  # noqa: E402
from sdrm_amd.engine import utility_engine  # noqa: E402

F = 8
SHAPES = {"ML-100k split": (943, 1008, 0.06, 95), "ML-1M shape": (6040, 3706, 0.04, 1208), "ADM shape": (5541, 3568, 0.0035, 554)}
PEAK_FLOPS, STORE_BW = 157.3e12, 6.29e12
FLOPS_PER_PAIR = 20 * F * F + 13 * F


def problem(name, seed=0):
    """(model on the GPU with weights of a trained model's size, training triples, validation triples, validation users, items)."""
    n_users, n_items, density, n_valid = SHAPES[name]
    rng = np.random.default_rng(seed)
    n = int(density * n_users * n_items)
    flat = rng.choice(n_users * n_items, size=n, replace=False)
    training = np.stack([flat // n_items, flat % n_items, rng.integers(0, 2, n)], axis=1).astype(np.int64)
    training = np.concatenate([training, np.stack([np.zeros(n_items, dtype=np.int64), np.arange(n_items), np.zeros(n_items, dtype=np.int64)], axis=1)])
    training = training[np.unique(training[:, 0] * n_items + training[:, 1], return_index=True)[1]]     # every item occurs; pairs unique
    users = np.sort(rng.choice(np.arange(1, n_users), size=n_valid, replace=False))
    seen = set((training[:, 0] * n_items + training[:, 1]).tolist())
    validation = [(u, i, 1) for u in users for i in rng.choice(n_items, size=20, replace=False) if u * n_items + i not in seen]
    torch.manual_seed(seed)
    model = neumf.NCF(n_users, n_items, factor=F).cuda().eval()
    with torch.no_grad():
        for p in model.parameters():       # a trained model's magnitudes rather than the initialisation's: no term vanishes
            p.copy_(torch.randn_like(p) * 0.3)
    return model, training, np.asarray(validation, dtype=np.int64), users, np.unique(training[:, 1])


def device_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def part_kernels(eng, lines):
    lines.append(f"{'kernels (F = 8)':<16}{'users x items':>14}{'call us':>10}{'k_neumf_stage':>15}{'k_neumf_scores':>16}{'TFLOP/s':>9}{'of fp32 peak':>14}{'store GB/s':>12}{'of 6.29 TB/s':>14}")
    for name in SHAPES:
        model, _, _, users, items = problem(name)
        w = model.engine_weights(eng.device)
        u, i = (torch.from_numpy(a.astype(np.int32)).cuda() for a in (users, items))
        out = torch.empty(len(users), len(items), dtype=torch.float32, device=eng.device)
        call = lambda: eng.neumf_scores(w, u, i, out=out, check=False)
        reps = max(20, int(2e9 / (len(users) * len(items) * FLOPS_PER_PAIR)) * 20)
        ms = device_ms(call, reps)
        eng.profile_begin(capacity=4096)
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        prof = eng.profile_end()
        stage = sum(v[0] / v[1] for k, v in prof.items() if "k_neumf_stage" in k)
        scores = sum(v[0] / v[1] for k, v in prof.items() if "k_neumf_scores" in k)
        kernel_s = ms * 1e-3 * scores / (stage + scores)       # the call's device time split by the profile's shares
        pairs = len(users) * len(items)
        lines.append(f"{name:<16}{f'{len(users)} x {len(items)}':>14}{ms * 1e3:>10.1f}{stage / (stage + scores):>14.0%} {scores / (stage + scores):>15.0%} "
                     f"{pairs * FLOPS_PER_PAIR / kernel_s / 1e12:>8.1f}{pairs * FLOPS_PER_PAIR / kernel_s / PEAK_FLOPS:>13.1%} {pairs * 4 / kernel_s / 1e9:>11.0f}"
                     f"{pairs * 4 / kernel_s / STORE_BW:>13.1%}   ({reps} calls timed)")
        print(lines[-1], flush=True)
        eng.feed_status()


@torch.no_grad()
def torch_matrix(model, u, i):
    pairs = torch.cartesian_prod(u, i)
    return torch.cat([model(pairs[s:s + neumf.EVAL_BATCH, 0], pairs[s:s + neumf.EVAL_BATCH, 1]) for s in range(0, pairs.shape[0], neumf.EVAL_BATCH)])


def part_torch(eng, lines):
    lines.append(f"{'torch, same GPU':<16}{'users x items':>14}{'torch ms':>10}{'engine ms':>11}{'torch / engine':>16}{'max |diff|':>12}")
    for name in SHAPES:
        model, _, _, users, items = problem(name)
        w = model.engine_weights(eng.device)
        u, i = (torch.from_numpy(a.astype(np.int32)).cuda() for a in (users, items))
        t_ms = device_ms(lambda: torch_matrix(model, u, i), reps=5, warmup=2)
        e_ms = device_ms(lambda: eng.neumf_scores(w, u, i, check=False), reps=50)
        diff = (torch_matrix(model, u, i).reshape(len(users), len(items)) - eng.neumf_scores(w, u, i)).abs().max().item()
        lines.append(f"{name:<16}{f'{len(users)} x {len(items)}':>14}{t_ms:>10.2f}{e_ms:>11.3f}{t_ms / e_ms:>15.0f}x{diff:>12.2e}")
        print(lines[-1], flush=True)


def pandas_evaluation(pd, model, training, validation, users):
    """The reference's testing block (neural_cf_benchmark_pt.py:294-332) in this project's words, on the model's device and the CPUs."""
    from sdrm_amd import metrics
    from scipy.sparse import csr_matrix
    train_df, valid_df = pd.DataFrame(training), pd.DataFrame(validation)
    with torch.no_grad():
        product = torch.cartesian_prod(torch.tensor(np.unique(users), device="cuda", dtype=torch.int32),
                                       torch.tensor(train_df[1].unique(), device="cuda", dtype=torch.int32))
        scores = []
        for s in range(0, product.shape[0], neumf.EVAL_BATCH):
            scores.extend(model(product[s:s + neumf.EVAL_BATCH, 0], product[s:s + neumf.EVAL_BATCH, 1]).cpu().numpy().flatten().tolist())
    frame = pd.DataFrame(product.cpu().numpy(), columns=[0, 1])
    frame["predictions"] = scores
    frame["validation_labels"] = frame.merge(valid_df, on=[0, 1], how="left")[2].fillna(0)
    frame["training_labels"] = frame.merge(train_df, on=[0, 1], how="left")[2]
    frame["masked"] = frame["predictions"].where(frame["training_labels"].isnull(), other=-np.inf)

    def through_dicts(column):
        rows = dict(zip(np.unique(frame[0]), range(frame[0].nunique())))
        cols = dict(zip(np.unique(frame[1]), range(frame[1].nunique())))
        return csr_matrix((frame[column], ([rows[x] for x in frame[0]], [cols[x] for x in frame[1]])), shape=(len(rows), len(cols)))
    actual, pred = through_dicts("validation_labels"), through_dicts("masked")
    rec = [np.round(np.nanmean(metrics.recall_at_k_batch(pred.toarray(), actual, k=k)), 4) for k in neumf.K_LIST]
    ndcg = [np.round(np.nanmean(metrics.NDCG_binary_at_k_batch(pred.toarray(), actual, k=k)), 4) for k in neumf.K_LIST]
    return np.array(rec), np.array(ndcg)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def part_full(eng, lines):
    try:
        import pandas as pd
    except ImportError:
        pd = None
        lines.append("pandas does not import here: the reference's procedure was not timed")
    lines.append(f"{'one evaluation':<16}{'users x items':>14}{'training rows':>15}{'pandas ms':>24}{'engine ms':>24}{'pandas / engine':>17}")
    for name in SHAPES:
        model, training, validation, users, items = problem(name)
        engine_call = lambda: neumf.rank_all_items(model, training, validation, users, eng)
        host_ms(engine_call)
        e = [host_ms(engine_call) for _ in range(5)]
        e_ms, (rec, ndcg) = float(np.median([t for t, _ in e])), e[-1][1]
        with np.errstate(invalid="ignore"):
            e_rec = np.array([np.round(np.nanmean(r), 4) for r in rec])
        cell_p, ratio, p_rec = "not timed", "", None
        if pd is not None:
            calls = 3 if name == "ML-100k split" else 1
            p = [host_ms(lambda: pandas_evaluation(pd, model, training, validation, users)) for _ in range(calls)]
            p_ms, p_rec = float(np.median([t for t, _ in p])), p[-1][1][0]
            cell_p, ratio = f"{p_ms:.0f} ({calls} call{'s' if calls > 1 else ''})", f"{p_ms / e_ms:.0f}x"
        lines.append(f"{name:<16}{f'{len(users)} x {len(items)}':>14}{training.shape[0]:>15}{cell_p:>24}{f'{e_ms:.1f} (median of 5)':>24}{ratio:>17}")
        lines.append(f"{'':<16}Recall@k engine {e_rec.tolist()}" + (f"  pandas {p_rec.tolist()}" if p_rec is not None else ""))
        print("\n".join(lines[-2:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernels", "torch", "full"), required=True)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "neumf_eval_bench needs the GPU"
    eng = utility_engine()
    lines = []
    {"kernels": part_kernels, "torch": part_torch, "full": part_full}[args.part](eng, lines)
    text = "\n".join(lines) + "\n\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The downstream truncated-SVD evaluator, host against device, one process, at two shapes:

  ML-100k fixture   tests/golden/ml100k.npz: train 843 x 1008, the synthetic part its rows permuted, the fixture's validation users
  ML-1M shape       synthetic interactions (synth.synth_feed_csr, fixed seeds): train and synthetic part 6034 x 3125 at 5 %, 604
                    validation users

  host     pipeline.compute_mf_results: sklearn's TruncatedSVD(20, n_iter=100) on the densified stack, numpy metrics; host clock
  device   pipeline.compute_mf_results_device END TO END - the split, the stacking, both uploads (CSR and CSC), the fit with its
           read-back and the host's closing eigenproblem, the scores, the ranking, the read-back of the per-user figures; host clock
           around a call that ends in a device synchronise

Both after warm-up calls, the variants alternating inside every round; the table gives the median call and the min .. max spread.
Then, from one more device call each: the kernel launches of the call (sdrm_launch_count) and, from the engine's event profile
(sdrm_profile_begin: two events around every launch, so each interval carries a few microseconds of marker cost - shares, not
durations), the share of every kernel class.

`--out FILE` also writes the tables there (profiles/svd_eval_bench.txt is such a file)."""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrm_amd import pipeline, synth  # noqa: E402
from sdrm_amd.engine import utility_engine  # noqa: E402

DEVICE_WARMUP, DEVICE_PER_ROUND = 3, 3
# host warm-up calls and timed host calls per shape: a host call at the ML-1M shape takes most of a minute, and sklearn and the BLAS
# under it are warm from the first shape
HOST_PLAN = {"ML-100k fixture": (1, 3), "ML-1M shape": (0, 2)}
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ml100k.npz")


def ml100k():
    z = np.load(GOLDEN)
    train, valid = pipeline.csr_from_npz(z, "train_test"), pipeline.csr_from_npz(z, "valid")
    train.eliminate_zeros()
    train.data[:] = 1.0
    return train, valid, train[np.random.RandomState(7).permutation(train.shape[0])].tocsr()


def ml1m_shape():
    mk = lambda rows, seed: synth.synth_feed_csr(rows, 3125, 0.05, seed=seed, ratings=False)
    return mk(6034, 7), mk(604, 8), mk(6034, 9)


def timed(fn):
    with contextlib.redirect_stdout(io.StringIO()):   # (the split prints a line per user it drops)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "svd_eval_bench needs the GPU"
    eng = utility_engine()
    lines = [f"{'SVD evaluator':<16}{'stack':>14}{'nnz':>9}{'host ms':>30}{'device ms':>26}{'host / device':>15}{'launches':>10}",
             "(median call, min .. max; host: %s timed calls after %s warm-up, sklearn on %s CPU threads; device: %d calls per host call after %d warm-up, end to "
             "end with uploads, read-backs and the host eigenproblem; variants alternating)"
             % (" / ".join(str(c) for _, c in HOST_PLAN.values()), " / ".join(str(w) for w, _ in HOST_PLAN.values()), os.environ.get("OMP_NUM_THREADS", "all"),
                DEVICE_PER_ROUND, DEVICE_WARMUP)]
    shares = []
    for name, (train, valid, synthetic) in (("ML-100k fixture", ml100k()), ("ML-1M shape", ml1m_shape())):
        host = lambda: pipeline.compute_mf_results(train, valid.copy(), synthetic, only_synthetic=True)
        device = lambda: pipeline.compute_mf_results_device(train, valid.copy(), synthetic, eng, only_synthetic=True, seed=0)
        host_warmup, host_calls = HOST_PLAN[name]
        for _ in range(host_warmup):
            timed(host)
        for _ in range(DEVICE_WARMUP):
            _, d_out = timed(device)
        t = {"host": [], "device": []}
        for _ in range(host_calls):
            ms, h_out = timed(host)
            t["host"].append(ms)
            for _ in range(DEVICE_PER_ROUND):
                t["device"].append(timed(device)[0])
        before = eng.launch_count()
        timed(device)
        launches = eng.launch_count() - before
        eng.profile_begin(capacity=4096)
        timed(device)
        prof = eng.profile_end()
        total = sum(ms for ms, _, _ in prof.values())
        shares.append((name, [(k, ms, n, ms / total) for k, (ms, n, _) in prof.items()]))
        med = {tag: float(np.median(v)) for tag, v in t.items()}
        cell = lambda tag: f"{med[tag]:10.1f} ({min(t[tag]):.1f} .. {max(t[tag]):.1f})"
        rows = synthetic.shape[0] + valid.shape[0]
        lines.append(f"{name:<16}{f'<= {rows} x {train.shape[1]}':>14}{synthetic.nnz + valid.nnz:>9}{cell('host'):>30}{cell('device'):>26}"
                     f"{med['host'] / med['device']:>14.0f}x{launches:>10}")
        lines.append(f"{'':<16}Recall@k host   {h_out[0].tolist()}  device {d_out[0].tolist()}")
        lines.append(f"{'':<16}NDCG@k   host   {h_out[1].tolist()}  device {d_out[1].tolist()}")
        print("\n".join(lines[-3:]), flush=True)
    lines += ["", f"{'kernel class (event profile of one device call)':<110}{'launches':>9}{'ms':>9}{'share':>8}"]
    for name, rows in shares:
        lines.append(name)
        for k, ms, n, share in sorted(rows, key=lambda r: -r[1]):
            lines.append(f"  {k[:106]:<108}{n:>9}{ms:>9.2f}{share:>8.1%}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

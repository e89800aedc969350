#!/usr/bin/env python3
"""The downstream NMF evaluator (`nnmf=True`), host against device, one process, at the two shapes of tools/svd_eval_bench.py:

  ML-100k fixture   tests/golden/ml100k.npz: train 843 x 1008, the synthetic part its rows permuted, the fixture's validation users
  ML-1M shape       synthetic interactions (synth.synth_feed_csr, fixed seeds): train and synthetic part 6034 x 3125 at 5 %, 604
                    validation users

and two measurements per shape:

  fit          host: `NMF(n_components=15, max_iter=50).fit_transform` of the densified stack (sklearn, NNDSVDa start included);
               device: Engine.nmf_fit on the resident CSR and CSC forms, start included (svd_fit of 15 components with its read-back,
               sdrm_nmf_init, then the 50 iterations queued in one call and the one read-back of n_iter and the violations)
  end to end   host: pipeline.compute_mf_results(nnmf=True); device: pipeline.compute_mf_results_device(nnmf=True) - the split, the
               stacking, both uploads, the fit, the scores, the ranking, the read-back of the per-user figures

Host clock around calls that end in a device synchronise, after warm-up calls, the variants alternating inside every round; the table gives
the median call and the min .. max spread.  Then the kernel launches of one device fit (sdrm_launch_count), per iteration and for the
start, and the share of every kernel class in one end-to-end device call (the engine's event profile: two events around every launch,
so each interval carries a few microseconds of marker cost - shares, not durations).

`--out FILE` also writes the tables there (profiles/nmf_eval_bench.txt is such a file)."""
import argparse
import contextlib
import io
import os
import sys
import time
import warnings

import numpy as np
import torch
from scipy.sparse import vstack

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrm_amd import metrics, pipeline  # noqa: E402
from sdrm_amd.engine import utility_engine  # noqa: E402
from svd_eval_bench import ml100k, ml1m_shape  # noqa: E402

DEVICE_WARMUP, DEVICE_PER_ROUND = 3, 3
HOST_PLAN = {"ML-100k fixture": (1, 3), "ML-1M shape": (0, 2)}   # host warm-up calls and timed host calls per shape
K, MAX_ITER = 15, 50


def timed(fn):
    with contextlib.redirect_stdout(io.StringIO()):   # (the split prints a line per user it drops)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out


def stacked(valid, synthetic):
    test_data, _ = metrics.split_train_test_proportion_from_csr_matrix(valid.copy(), batch_size=1000, random_seed=123)
    combined = vstack([synthetic.astype(np.float64), test_data.astype(np.float64)]).tocsr()
    combined.eliminate_zeros()
    return combined


def host_fit(dense):
    from sklearn.decomposition import NMF
    from sklearn.exceptions import ConvergenceWarning
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=ConvergenceWarning)
        model = NMF(n_components=K, max_iter=MAX_ITER)
        model.fit_transform(dense)
    return model.n_iter_


def measure(host, device, name):
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
    med = {tag: float(np.median(v)) for tag, v in t.items()}
    cell = lambda tag: f"{med[tag]:10.1f} ({min(t[tag]):.1f} .. {max(t[tag]):.1f})"
    return cell("host"), cell("device"), med["host"] / med["device"], h_out, d_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "nmf_eval_bench needs the GPU"
    eng = utility_engine()
    lines = [f"{'NMF evaluator':<16}{'what':<12}{'stack':>14}{'nnz':>9}{'host ms':>32}{'device ms':>28}{'host / device':>15}",
             "(median call, min .. max; host: %s timed calls after %s warm-up, sklearn on %s CPU threads; device: %d calls per host call after %d warm-up; "
             "variants alternating)"
             % (" / ".join(str(c) for _, c in HOST_PLAN.values()), " / ".join(str(w) for w, _ in HOST_PLAN.values()), os.environ.get("OMP_NUM_THREADS", "all"),
                DEVICE_PER_ROUND, DEVICE_WARMUP)]
    shares, counts = [], []
    for name, (train, valid, synthetic) in (("ML-100k fixture", ml100k()), ("ML-1M shape", ml1m_shape())):
        combined = stacked(valid, synthetic)
        dense = combined.toarray()
        csr_dev, csc_dev = eng.csr_to_device(combined), eng.csc_to_device(combined)
        shape = f"{combined.shape[0]} x {combined.shape[1]}"
        h, d, ratio, h_iter, d_out = measure(lambda: host_fit(dense), lambda: eng.nmf_fit(csr_dev, csc_dev, n_components=K, max_iter=MAX_ITER, seed=0), name)
        lines.append(f"{name:<16}{'fit':<12}{shape:>14}{combined.nnz:>9}{h:>32}{d:>28}{ratio:>14.1f}x")
        lines.append(f"{'':<16}n_iter host {h_iter}, device {d_out[2]}; violation v_n / v_1 on the device {d_out[3][-1] / d_out[3][0]:.3e}")
        print("\n".join(lines[-2:]), flush=True)
        # launches: a fit from a custom start is the iterations alone
        w0, h0 = eng.nmf_init(csr_dev, csc_dev, n_components=K, seed=0)
        before = eng.launch_count()
        eng.nmf_fit(csr_dev, csc_dev, n_components=K, max_iter=MAX_ITER, init=(w0, h0))
        per_fit = eng.launch_count() - before
        before = eng.launch_count()
        eng.nmf_init(csr_dev, csc_dev, n_components=K, seed=0)
        counts.append((name, per_fit, per_fit / MAX_ITER, eng.launch_count() - before))
        host = lambda: pipeline.compute_mf_results(train, valid.copy(), synthetic, only_synthetic=True, nnmf=True)
        device = lambda: pipeline.compute_mf_results_device(train, valid.copy(), synthetic, eng, only_synthetic=True, seed=0, nnmf=True)
        h, d, ratio, h_out, d_out = measure(host, device, name)
        lines.append(f"{name:<16}{'end to end':<12}{shape:>14}{combined.nnz:>9}{h:>32}{d:>28}{ratio:>14.1f}x")
        lines.append(f"{'':<16}Recall@k host   {h_out[0].tolist()}  device {d_out[0].tolist()}")
        lines.append(f"{'':<16}NDCG@k   host   {h_out[1].tolist()}  device {d_out[1].tolist()}")
        print("\n".join(lines[-3:]), flush=True)
        eng.profile_begin(capacity=4096)
        timed(device)
        prof = eng.profile_end()
        total = sum(ms for ms, _, _ in prof.values())
        shares.append((name, [(k, ms, n, ms / total) for k, (ms, n, _) in prof.items()]))
    lines += ["", "kernel launches (sdrm_launch_count)"]
    for name, per_fit, per_iter, start in counts:
        lines.append(f"  {name:<16}{MAX_ITER} iterations from a given start: {per_fit} ({per_iter:g} per iteration: product + Gram, sweep for W and for H, the stop rule); "
                     f"the start (svd_fit of {K} components + sdrm_nmf_init): {start}")
    lines += ["", f"{'kernel class (event profile of one end-to-end device call)':<110}{'launches':>9}{'ms':>9}{'share':>8}"]
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

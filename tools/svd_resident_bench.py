#!/usr/bin/env python3
"""The device SVD evaluator from a score matrix that is on the device - what a run holds after sampling - by two paths, one process,
at the two stacks of tools/svd_eval_bench.py (the ML-100k fixture; the ML-1M shape, 6638 x 3125 with 1.04 M entries):

  parent     pipeline.equal_sparsity_csr (the CSR made on the device, copied to the host) + pipeline.compute_mf_results_device (scipy's
             vstack, the CSR upload, the host's tocsc() and the CSC upload)
  resident   Engine.equal_sparsity_csr (the CSR stays on the device) + pipeline.compute_mf_results_resident (Engine.csr_vstack and
             Engine.csr_transpose; only the split of the validation users is uploaded)

`raw` is the synthetic 0/1 matrix plus uniform noise in [0, 0.25): at the data's sparsity quantile the binarisation gives the synthetic
matrix back (to within a few entries at 2 x 10^7 elements: np.quantile's float32 rank), so both paths fit the stack svd_eval_bench.py
fits.  Host clock around calls that end in a device synchronise, after warm-up calls, the two paths alternating; the table gives the median call and the min .. max spread, and the two results must be equal.  Then,
from one more resident call, the engine's event profile (two events around every launch: each interval carries a few microseconds of
marker cost) of the new kernels, per launch.

Last, the two forms of the transpose's mark pass (64-bit global atomics into a cleared table; column tiles in LDS), forced through
`Engine.debug_set(csrt_mark=...)` on the two stacks and on two wider matrices (4 and 9 LDS tiles), alternating, from the event profile:
per launch, the mark pass (the global form's interval holds its clearing) and the four launches of the transpose together.

`--out FILE` also writes the tables there (profiles/svd_resident_bench.txt is such a file)."""
import argparse
import os
import sys

import numpy as np
import torch
from scipy.sparse import vstack

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrm_amd import pipeline, synth  # noqa: E402
from sdrm_amd.engine import utility_engine  # noqa: E402
from svd_eval_bench import ml100k, ml1m_shape, timed  # noqa: E402

WARMUP, ROUNDS = 3, 10
FORM_ROUNDS, FORM_CALLS = 5, 8
FORMS = (("global atomics", 1), ("LDS tiles", 2))


def mark_forms(eng, name, matrix):
    """One table line: median over the rounds of the per-launch microseconds of the mark pass and of the whole transpose, per form."""
    dev = eng.csr_to_device(matrix)
    t = {form: ([], []) for form, _ in FORMS}
    for form, mode in FORMS:                       # warm-up: code objects, scratch growth
        eng.debug_set(csrt_mark=mode)
        eng.csr_transpose(dev)
    for _ in range(FORM_ROUNDS):
        for form, mode in FORMS:
            eng.debug_set(csrt_mark=mode)
            eng.profile_begin(capacity=4096)
            for _ in range(FORM_CALLS):
                eng.csr_transpose(dev, check=False)
            prof = {k: v for k, v in eng.profile_end().items() if k.startswith("csr transpose")}
            t[form][0].append(1e3 * sum(ms for k, (ms, _, _) in prof.items() if "k_csrt_mark" in k) / FORM_CALLS)
            t[form][1].append(1e3 * sum(ms for ms, _, _ in prof.values()) / FORM_CALLS)
    eng.debug_set(csrt_mark=0)
    eng.feed_status()
    tiles = -(-matrix.shape[1] // 4096)
    cells = "".join(f"{np.median(t[form][0]):>24.1f}{np.median(t[form][1]):>13.1f}" for form, _ in FORMS)
    return f"{name:<18}{f'{matrix.shape[0]} x {matrix.shape[1]}':>14}{matrix.nnz:>9}{tiles:>7}{cells}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "svd_resident_bench needs the GPU"
    eng = utility_engine()
    lines = [f"{'SVD evaluator':<16}{'stack':>14}{'nnz':>9}{'parent ms':>28}{'resident ms':>28}{'parent / resident':>19}",
             f"(from a device score matrix to the twelve means, end to end; median call, min .. max of {ROUNDS} calls each after {WARMUP} warm-up, "
             "the two paths alternating)"]
    kernels, stacks = [], []
    for name, (train, valid, synthetic) in (("ML-100k fixture", ml100k()), ("ML-1M shape", ml1m_shape())):
        stacks.append(vstack([synthetic, valid]).tocsr())   # (the shape of the fitted stack: the split keeps 80 % of `valid`'s entries)
        noise = np.random.RandomState(1).random_sample(synthetic.shape) * 0.25
        raw = torch.from_numpy((synthetic.toarray() + noise).astype(np.float32)).to(eng.device)
        sparsity = 1 - synthetic.nnz / (synthetic.shape[0] * synthetic.shape[1])
        parent = lambda: pipeline.compute_mf_results_device(train, valid.copy(), pipeline.equal_sparsity_csr(raw, sparsity, eng), eng,
                                                            only_synthetic=True, seed=0)
        resident = lambda: pipeline.compute_mf_results_resident(train, valid.copy(), eng.equal_sparsity_csr(raw, sparsity), eng,
                                                                only_synthetic=True, seed=0)
        made = eng.equal_sparsity_csr(raw, sparsity)[1].numel()   # (np.quantile's float32 rank may sit a few entries beside nnz at 2 x 10^7 elements)
        assert abs(made - synthetic.nnz) <= 8, (made, synthetic.nnz)
        for _ in range(WARMUP):
            _, p_out = timed(parent)
            _, r_out = timed(resident)
        assert all(np.array_equal(p, r) for p, r in zip(p_out, r_out)), (p_out, r_out)
        t = {"parent": [], "resident": []}
        for _ in range(ROUNDS):
            t["parent"].append(timed(parent)[0])
            t["resident"].append(timed(resident)[0])
        eng.profile_begin(capacity=4096)
        timed(resident)
        prof = eng.profile_end()
        kernels.append((name, [(k, ms, n) for k, (ms, n, _) in prof.items() if k.startswith(("csr transpose", "csr vstack"))],
                        sum(ms for ms, _, _ in prof.values())))
        med = {tag: float(np.median(v)) for tag, v in t.items()}
        cell = lambda tag: f"{med[tag]:10.1f} ({min(t[tag]):.1f} .. {max(t[tag]):.1f})"
        rows = synthetic.shape[0] + valid.shape[0]
        lines.append(f"{name:<16}{f'<= {rows} x {train.shape[1]}':>14}{synthetic.nnz + valid.nnz:>9}{cell('parent'):>28}{cell('resident'):>28}"
                     f"{med['parent'] / med['resident']:>18.2f}x")
        lines.append(f"{'':<16}Recall@k parent {p_out[0].tolist()}  resident {r_out[0].tolist()}")
        print("\n".join(lines[-2:]), flush=True)
    lines += ["", f"{'new kernels (event profile of one resident call)':<110}{'launches':>9}{'us / launch':>13}"]
    for name, rows, total in kernels:
        lines.append(f"{name} (all launches of the call: {total:.2f} ms)")
        for k, ms, n in rows:
            lines.append(f"  {k[:106]:<108}{n:>9}{1e3 * ms / n:>13.1f}")
    wide = lambda rows, cols, density, seed: synth.synth_feed_csr(rows, cols, density, seed=seed, ratings=False)
    lines += ["", f"{'mark pass of csr_transpose':<18}{'matrix':>14}{'nnz':>9}{'tiles':>7}" + "".join(f"{form + ' mark us':>24}{'all four us':>13}" for form, _ in FORMS),
              f"(per launch, from the event profile; median of {FORM_ROUNDS} rounds of {FORM_CALLS} calls, the forms alternating)"]
    for name, matrix in (("ML-100k stack", stacks[0]), ("ML-1M stack", stacks[1]), ("4 tiles", wide(4096, 16384, 0.01, 11)), ("9 tiles", wide(4096, 36864, 0.005, 12))):
        lines.append(mark_forms(eng, name, matrix))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

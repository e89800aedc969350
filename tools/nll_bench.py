#!/usr/bin/env python3
"""The loss head of the MultiVAE++ pre-stage (train_SDRM.py:141-142) and one pre-stage epoch, one process.

Part 1, forward + backward of the loss head on the same logits, HIP events, two ways:

  torch    -mean(sum(log_softmax(o) * X)) on a dense X, then .backward() to o.grad
  engine   sdrm_multinomial_nll_csr + sdrm_multinomial_nll_csr_grad (scale = a device scalar holding 1), no dense X

at the VAE batch and item counts of the three BASELINE configurations and at the largest published batch (870 x 8582).  Warm-up,
then WINDOWS timed windows per variant, the variants alternating inside every round; the table gives the median window and the
min .. max spread in us per call, and the engine pair's 12 B per element over its median as GB/s.

Part 2, `train_variational_autoencoder` for EPOCHS epochs with and without `device_feed`, host clock around a call that ends in
a device synchronise, alternating, ms per epoch (train half + evaluation half, checkpoint writes included in both).

`--out FILE` also writes the tables there (profiles/multinomial_nll_bench.txt is such a file)."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrm_amd import synth  # noqa: E402
from sdrm_amd.engine import utility_engine  # noqa: E402
from sdrm_amd.vae_hooks import VAE, train_variational_autoencoder  # noqa: E402
from encode_bench import ml100k_rows, window  # noqa: E402

# name, batch, n_items, density (None: the real ML-100k rows), ratings
HEAD_SHAPES = [
    ("ML-100k/SVD B=780", 780, 1008, None, True),
    ("ML-1M/MLP B=310", 310, 3125, 0.05, True),
    ("ADM/NeuMF B=290", 290, 8582, 0.012, False),
    ("largest B=870", 870, 8582, 0.012, False),
]
# name, users, n_items, density, ratings, hidden, latent, batch
EPOCH_SHAPES = [
    ("ML-100k/SVD", 843, 1008, None, True, 930, 830, 780),
    ("ML-1M/MLP", 6034, 3125, 0.05, True, 20, 20, 310),
    ("ADM/NeuMF", 10621, 8582, 0.012, False, 40, 40, 290),
]
WINDOWS, WARMUP, REPS, EPOCHS, EPOCH_WINDOWS = 7, 5, 100, 2, 3


def feed(n_rows, n_items, density, ratings):
    return ml100k_rows() if density is None else synth.synth_feed_csr(n_rows, n_items, density, seed=7, ratings=ratings)


def head_table(eng):
    lines = [f"{'loss head, fwd + bwd':<22}{'nnz/row':>8}{'torch us':>24}{'engine us':>24}{'engine GB/s':>12}   fastest",
             "(median of %d windows of %d calls, min .. max; variants alternating; 12 B per element for the engine pair)" % (WINDOWS, REPS)]
    for name, b, n_items, density, ratings in HEAD_SHAPES:
        m = feed(max(b, 843), n_items, density, ratings)[:b]
        csr = eng.csr_to_device(m)
        x = eng.csr_rows_to_dense(csr, row0=0, b=b)
        o = (torch.randn(b, n_items, device="cuda", generator=torch.Generator("cuda").manual_seed(3)) * 2).requires_grad_()
        up = torch.ones(1, dtype=torch.float32, device="cuda")   # the upstream gradient autograd hands the head in the pre-stage

        def v_torch():
            o.grad = None
            (-torch.mean(torch.sum(F.log_softmax(o, dim=1) * x, dim=1))).backward()
            return o.grad

        def v_engine():
            od = o.detach()
            _, lse = eng.multinomial_nll_csr(od, csr, row0=0, b=b, check=False)
            return eng.multinomial_nll_csr_grad(od, lse, csr, row0=0, b=b, scale=up)
        variants = [("torch", v_torch), ("engine", v_engine)]
        ref = v_torch().double().clone()
        err = float((v_engine().double() - ref).abs().max() / ref.abs().max())   # faster and different is not faster
        assert err <= 1e-4, (name, err)
        for _, fn in variants:
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        t = {tag: [] for tag, _ in variants}
        for _ in range(WINDOWS):
            for tag, fn in variants:
                t[tag].append(window(fn, REPS))
        eng.feed_status()
        med = {tag: float(np.median(v)) for tag, v in t.items()}
        cell = lambda tag: f"{med[tag]:8.1f} ({min(t[tag]):.1f} .. {max(t[tag]):.1f})"
        lines.append(f"{name:<22}{m.nnz / b:>8.0f}{cell('torch'):>24}{cell('engine'):>24}{12.0 * b * n_items / med['engine'] / 1e3:>12.0f}   {min(med, key=med.get)}")
        print(lines[-1], flush=True)
    return lines


def epoch_table():
    lines = [f"{'pre-stage epoch':<22}{'batches':>8}{'default ms':>26}{'device_feed ms':>26}   fastest",
             "(%d epochs per call, median of %d calls, min .. max, per epoch; host clock to a device synchronise; calls alternating)" % (EPOCHS, EPOCH_WINDOWS)]
    for name, users, n_items, density, ratings, hidden, latent, batch in EPOCH_SHAPES:
        m = feed(users, n_items, density, ratings)

        def epochs_ms(flag):
            torch.manual_seed(5)
            np.random.seed(6)
            vae = VAE(n_items, hidden, latent).cuda()
            with tempfile.TemporaryDirectory() as where:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                train_variational_autoencoder(vae, m, m, EPOCHS, batch, 1e-3, "Recall@10", where, device_feed=flag)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / EPOCHS
        for flag in (False, True):   # warm-up: code objects, rocBLAS picks, the allocator's pools
            epochs_ms(flag)
        t = {False: [], True: []}
        for _ in range(EPOCH_WINDOWS):
            for flag in (False, True):
                t[flag].append(epochs_ms(flag))
        med = {flag: float(np.median(v)) for flag, v in t.items()}
        cell = lambda flag: f"{med[flag]:9.1f} ({min(t[flag]):.1f} .. {max(t[flag]):.1f})"
        lines.append(f"{name:<22}{-(-m.shape[0] // batch):>8}{cell(False):>26}{cell(True):>26}   {'device_feed' if med[True] < med[False] else 'default'}")
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "nll_bench needs the GPU"
    text = "\n".join(head_table(utility_engine()) + [""] + epoch_table()) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The train-mode input layer of the VAE encoder (train_SDRM.py:242-244, first Linear, forward and weight gradient) and one
pre-stage epoch, one process.

Part 1, forward + backward of the input layer for one batch, HIP events, two ways:

  dense    what `device_feed=True` alone runs: csr_rows_to_dense, then F.normalize -> F.dropout -> F.linear and .backward() to
           W1.grad and b1.grad (torch's generator draws the mask)
  engine   sdrm_vae_input_layer_fwd + dpre.sum(0) + sdrm_vae_input_layer_wgrad, no dense batch (Philox draws the mask)

at the four shapes of the encode hook's table, p_drop = 0.5, the batch a slice of a random order of the feed.  Warm-up,
then WINDOWS timed windows per variant, the variants alternating inside every round; the table gives the median window and the
min .. max spread in us per batch, and the engine's two kernels on their own.

Part 2, `train_variational_autoencoder` for EPOCHS epochs with `device_feed=True`, with and without `sparse_input=True`, host clock
around a call that ends in a device synchronise, alternating, ms per epoch (train half + evaluation half, checkpoints included).

`--out FILE` also writes the tables there (profiles/vae_input_layer_bench.txt is such a file)."""
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
from sdrm_amd.vae_hooks import VAE, SparseFeed, train_variational_autoencoder  # noqa: E402
from encode_bench import SHAPES, ml100k_rows, window  # noqa: E402

# name, users, n_items, density, ratings, hidden, latent, batch: the pre-stage of the three BASELINE configurations
EPOCH_SHAPES = [
    ("ML-100k/SVD", 843, 1008, None, True, 930, 830, 780),
    ("ML-1M/MLP", 6034, 3125, 0.05, True, 600, 340, 310),
    ("ADM/NeuMF", 10621, 8582, 0.012, False, 200, 40, 290),
]
WINDOWS, WARMUP, REPS, EPOCHS, EPOCH_WINDOWS, P_DROP = 7, 5, 50, 2, 3, 0.5


def feed_matrix(n_rows, n_items, density, ratings):
    return ml100k_rows() if density is None else synth.synth_feed_csr(n_rows, n_items, density, seed=7, ratings=ratings)


def layer_table(eng):
    lines = [f"{'input layer, fwd + bwd':<18}{'nnz':>9}{'dense us':>26}{'engine us':>26}{'fwd us':>9}{'wgrad us':>10}   fastest",
             "(median of %d windows of %d batches, min .. max; variants alternating; p_drop %.1f)" % (WINDOWS, REPS, P_DROP)]
    for name, n_rows, n_items, density, ratings, hidden, _, batch in SHAPES:
        m = feed_matrix(n_rows, n_items, density, ratings)
        batch = min(batch, m.shape[0])
        feed = SparseFeed(m, engine=eng)
        feed.set_order(np.random.RandomState(9).permutation(m.shape[0]))
        lo = min(batch, m.shape[0] - batch)
        rows = feed.order[lo:lo + batch]
        gen = torch.Generator("cuda").manual_seed(3)
        w1 = (torch.randn(hidden, n_items, device="cuda", generator=gen) / n_items ** 0.5).requires_grad_()
        b1 = torch.zeros(hidden, device="cuda").requires_grad_()
        dpre = torch.randn(batch, hidden, device="cuda", generator=gen)
        kw = dict(seed=11, step=3, p_drop=P_DROP, check=False)

        def v_dense():
            w1.grad = b1.grad = None
            x = eng.csr_rows_to_dense(feed.csr, rows=rows, check=False)
            F.linear(F.dropout(F.normalize(x, p=2, dim=1), P_DROP, True), w1, b1).backward(dpre)
            return w1.grad

        def v_fwd():
            return eng.vae_input_layer_fwd(w1.detach(), b1.detach(), feed.csr, rows=rows, **kw)

        rowscale = v_fwd()[1]

        def v_wgrad():
            return eng.vae_input_layer_wgrad(dpre, rowscale, feed.csc, pos=feed.pos, lo=lo, b=batch, **kw)

        def v_engine():
            _, rs = v_fwd()
            dpre.sum(0)
            return eng.vae_input_layer_wgrad(dpre, rs, feed.csc, pos=feed.pos, lo=lo, b=batch, **kw)

        # faster and different is not faster: without dropout the two ways compute the same gradient
        x = eng.csr_rows_to_dense(feed.csr, rows=rows)
        w1.grad = None
        F.linear(F.normalize(x, p=2, dim=1), w1, b1).backward(dpre)
        _, rs0 = eng.vae_input_layer_fwd(w1.detach(), b1.detach(), feed.csr, rows=rows, seed=11, step=3, p_drop=0.0)
        g0 = eng.vae_input_layer_wgrad(dpre, rs0, feed.csc, pos=feed.pos, lo=lo, b=batch, seed=11, step=3, p_drop=0.0)
        err = float((g0.double() - w1.grad.double()).abs().max() / w1.grad.double().abs().max())
        assert err <= 1e-4, (name, err)
        variants = [("dense", v_dense), ("engine", v_engine), ("fwd", v_fwd), ("wgrad", v_wgrad)]
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
        lines.append(f"{name:<18}{m.nnz:>9}{cell('dense'):>26}{cell('engine'):>26}{med['fwd']:>9.1f}{med['wgrad']:>10.1f}   "
                     f"{'engine' if med['engine'] < med['dense'] else 'dense'}")
        print(lines[-1], flush=True)
    return lines


def epoch_table():
    lines = [f"{'pre-stage epoch':<18}{'batches':>8}{'device_feed ms':>28}{'+ sparse_input ms':>28}   fastest",
             "(%d epochs per call, median of %d calls, min .. max, per epoch; host clock to a device synchronise; calls alternating)" % (EPOCHS, EPOCH_WINDOWS)]
    for name, users, n_items, density, ratings, hidden, latent, batch in EPOCH_SHAPES:
        m = feed_matrix(users, n_items, density, ratings)

        def epochs_ms(flag):
            torch.manual_seed(5)
            np.random.seed(6)
            vae = VAE(n_items, hidden, latent).cuda()
            with tempfile.TemporaryDirectory() as where:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                train_variational_autoencoder(vae, m, m, EPOCHS, batch, 1e-3, "Recall@10", where, device_feed=True, sparse_input=flag)
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
        lines.append(f"{name:<18}{-(-m.shape[0] // batch):>8}{cell(False):>28}{cell(True):>28}   {'sparse_input' if med[True] < med[False] else 'device_feed'}")
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "input_layer_bench needs the GPU"
    text = "\n".join(layer_table(utility_engine()) + [""] + epoch_table()) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

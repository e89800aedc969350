#!/usr/bin/env python3
"""The per-user hold-out split of the MultiVAE++ pre-stage (utilities.py:174-236) and one pre-stage epoch, one process, at the
three EPOCH_SHAPES of tools/nll_bench.py (the same synthetic feeds, the same seeds).

Part 1, the split alone, two ways:

  host     metrics.split_train_test_proportion_from_csr_matrix(test_data), host clock, one call per window
  engine   Engine.holdout_split (sdrm_holdout_split, csrc/holdout.h) on the resident CSR, HIP events, REPS calls per window

WINDOWS windows per variant, the variants alternating inside every round; the table gives the median window and the min .. max
spread per call.

Part 2, `train_variational_autoencoder(device_feed=True)` for EPOCHS epochs without and with `device_holdout=True`, under the epoch
protocol of nll_bench.epoch_table: host clock around a call that ends in a device synchronise, calls alternating, ms per epoch
(train half + evaluation half, checkpoint writes included in both).

Part 3, what is left of such an epoch: `evaluate_holdout` alone and one `checkpoint` write, host clock to a device synchronise.

`--out FILE` also writes the tables there (profiles/holdout_split_bench.txt is such a file)."""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrm_amd import metrics  # noqa: E402
from sdrm_amd.engine import utility_engine  # noqa: E402
from sdrm_amd.vae_hooks import VAE, checkpoint, evaluate_holdout, train_variational_autoencoder  # noqa: E402
from encode_bench import window  # noqa: E402
from nll_bench import EPOCH_SHAPES, EPOCH_WINDOWS, EPOCHS, WINDOWS, feed  # noqa: E402

REPS, WARMUP = 20, 3


def split_table(eng):
    lines = [f"{'hold-out split':<14}{'users':>7}{'nnz/row':>8}{'longest':>8}{'> 256':>7}{'host ms':>26}{'engine us':>26}{'host / engine':>15}",
             "(median of %d windows, min .. max, per call; host: one call per window, host clock; engine: %d calls per window, HIP events; "
             "variants alternating; > 256: rows of the work-group form)" % (WINDOWS, REPS)]
    for name, users, n_items, density, ratings, _, _, _ in EPOCH_SHAPES:
        m = feed(users, n_items, density, ratings)
        csr = eng.csr_to_device(m)
        n = np.diff(m.indptr)

        def v_host():
            with contextlib.redirect_stdout(io.StringIO()):
                t0 = time.perf_counter()
                metrics.split_train_test_proportion_from_csr_matrix(m, batch_size=1000)
                return (time.perf_counter() - t0) * 1e3
        draw = [0]

        def v_engine():
            draw[0] += 1
            return eng.holdout_split(csr, seed=7, draw=draw[0], check=False)
        np.random.seed(6)
        v_host()
        for _ in range(WARMUP):
            v_engine()
        torch.cuda.synchronize()
        t = {"host": [], "engine": []}
        for _ in range(WINDOWS):
            t["host"].append(v_host())
            t["engine"].append(window(v_engine, REPS))
        eng.feed_status()
        med = {tag: float(np.median(v)) for tag, v in t.items()}
        cell = lambda tag: f"{med[tag]:9.1f} ({min(t[tag]):.1f} .. {max(t[tag]):.1f})"
        lines.append(f"{name:<14}{m.shape[0]:>7}{m.nnz / m.shape[0]:>8.0f}{int(n.max()):>8}{int((n > 256).sum()):>7}{cell('host'):>26}{cell('engine'):>26}"
                     f"{med['host'] * 1e3 / med['engine']:>14.0f}x")
        print(lines[-1], flush=True)
    return lines


def epoch_table():
    lines = [f"{'pre-stage epoch':<14}{'batches':>8}{'device_feed ms':>28}{'+ device_holdout ms':>28}   fastest",
             "(%d epochs per call, median of %d calls, min .. max, per epoch; host clock to a device synchronise; calls alternating)" % (EPOCHS, EPOCH_WINDOWS)]
    for name, users, n_items, density, ratings, hidden, latent, batch in EPOCH_SHAPES:
        m = feed(users, n_items, density, ratings)

        def epochs_ms(flag):
            torch.manual_seed(5)
            np.random.seed(6)
            vae = VAE(n_items, hidden, latent).cuda()
            with tempfile.TemporaryDirectory() as where, contextlib.redirect_stdout(io.StringIO()):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                train_variational_autoencoder(vae, m, m, EPOCHS, batch, 1e-3, "Recall@10", where, device_feed=True, device_holdout=flag)
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
        lines.append(f"{name:<14}{-(-m.shape[0] // batch):>8}{cell(False):>28}{cell(True):>28}   {'device_holdout' if med[True] < med[False] else 'device_feed'}")
        print(lines[-1], flush=True)
    return lines


def parts_table(eng):
    lines = [f"{'parts of an epoch':<18}{'evaluate_holdout ms':>28}{'checkpoint ms':>28}",
             "(median of %d calls after a warm-up, min .. max; host clock to a device synchronise)" % WINDOWS]
    for name, users, n_items, density, ratings, hidden, latent, _ in EPOCH_SHAPES:
        csr = eng.csr_to_device(feed(users, n_items, density, ratings))
        torch.manual_seed(5)
        vae = VAE(n_items, hidden, latent).cuda()
        with tempfile.TemporaryDirectory() as where:
            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            variants = {"eval": lambda: evaluate_holdout(vae, eng, csr, 7, 1, "Recall@10"), "ckpt": lambda: checkpoint(vae, "epoch-0.pth", where)}
            t = {tag: [timed(fn) for _ in range(WINDOWS + 1)][1:] for tag, fn in variants.items()}
        eng.feed_status()
        cell = lambda tag: f"{float(np.median(t[tag])):9.1f} ({min(t[tag]):.1f} .. {max(t[tag]):.1f})"
        lines.append(f"{name:<18}{cell('eval'):>28}{cell('ckpt'):>28}")
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "holdout_bench needs the GPU"
    text = "\n".join(split_table(utility_engine()) + [""] + epoch_table() + [""] + parts_table(utility_engine())) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Adam on the device (csrc/vae_adam.h) and the train step without autograd, one process, at the three EPOCH_SHAPES of
tools/input_layer_bench.py.

Part 1, the optimizer alone on the model's eight tensors, two ways:

  torch    what the pre-stage runs without `device_optimizer`: `optimizer.zero_grad(); optimizer.step()` of `torch.optim.Adam(lr)` in
           its default form (the gradients are put back before every call: `zero_grad` sets them to None)
  engine   `DeviceAdam.zero_grad(); DeviceAdam.step()`: one launch of k_vae_adam

Device time by HIP events and wall time by the host clock to a device synchronise, both per call: warm-up, then WINDOWS timed windows
per variant, the variants alternating inside every round; the table gives the median window and the min .. max spread in us.  Before
timing, the two ways are compared on one step from equal state at 1e-4 of the largest update.

Part 2, `train_variational_autoencoder` with the five flags `device_feed, sparse_input, device_holdout, device_latent, device_decoder`
for EPOCHS epochs, three ways: as it stands without `device_optimizer`, with it on the autograd path (`DIRECT_STEP = False`), and with
it on the direct step (`vae_train_step`).  Host clock around a call that ends in a device synchronise, calls alternating, ms per epoch
(train half + evaluation half, checkpoint writes included in all three) and per batch.

`--out FILE` also writes the tables there (profiles/vae_optimizer_bench.txt is such a file)."""
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
from sdrm_amd import vae_hooks  # noqa: E402
from sdrm_amd.engine import utility_engine  # noqa: E402
from sdrm_amd.vae_hooks import VAE, DeviceAdam, train_variational_autoencoder  # noqa: E402
from encode_bench import window  # noqa: E402
from input_layer_bench import EPOCH_SHAPES, EPOCH_WINDOWS, EPOCHS, REPS, WARMUP, WINDOWS, feed_matrix  # noqa: E402


def wall_window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def optimizer_table(eng):
    lines = [f"{'optimizer alone':<14}{'elements':>10}{'chunks':>8}{'torch device us':>26}{'engine device us':>26}{'torch wall us':>26}{'engine wall us':>26}",
             "(median of %d windows of %d calls, min .. max; variants alternating)" % (WINDOWS, REPS)]
    for name, _, n_items, _, _, hidden, latent, _ in EPOCH_SHAPES:
        def fresh():
            torch.manual_seed(4)
            model = VAE(n_items, hidden, latent).cuda()
            gen = torch.Generator("cuda").manual_seed(3)
            return model, [torch.randn(p.shape, device="cuda", generator=gen) * 0.01 for p in model.parameters()]

        model_t, grads = fresh()
        model_e, _ = fresh()
        params_t, params_e = list(model_t.parameters()), list(model_e.parameters())
        opt_t = torch.optim.Adam(params_t, lr=1e-3)
        opt_e = DeviceAdam(model_e.named_parameters(), lr=1e-3, engine=eng)

        def v_torch():
            opt_t.zero_grad()
            for p, g in zip(params_t, grads):
                p.grad = g
            opt_t.step()

        def v_engine():
            opt_e.zero_grad()
            for p, g in zip(params_e, grads):
                p.grad = g
            opt_e.step()

        # faster and different is not faster: one step from equal state, at 1e-4 of the largest update
        start = [p.detach().clone() for p in params_t]
        v_torch()
        v_engine()
        for p0, a, b in zip(start, params_t, params_e):
            upd = float((a.detach() - p0).abs().max())
            err = float((a.detach() - b.detach()).abs().max())
            assert upd > 0 and err <= 2.0 ** -24 * float(a.detach().abs().max()) + 1e-4 * upd, (name, err, upd)
        variants = [("torch", v_torch), ("engine", v_engine)]
        for _, fn in variants:
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        dev = {tag: [] for tag, _ in variants}
        wall = {tag: [] for tag, _ in variants}
        for _ in range(WINDOWS):
            for tag, fn in variants:
                dev[tag].append(window(fn, REPS))
            for tag, fn in variants:
                wall[tag].append(wall_window(fn, REPS))
        cell = lambda t, tag: f"{float(np.median(t[tag])):8.1f} ({min(t[tag]):.1f} .. {max(t[tag]):.1f})"
        n = sum(p.numel() for p in params_t)
        chunks = sum(-(-p.numel() // vae_hooks.ADAM_CHUNK) for p in params_t)
        lines.append(f"{name:<14}{n:>10}{chunks:>8}{cell(dev, 'torch'):>26}{cell(dev, 'engine'):>26}{cell(wall, 'torch'):>26}{cell(wall, 'engine'):>26}")
        print(lines[-1], flush=True)
    return lines


def epoch_table():
    ways = (("five flags", dict(), True), ("+ device_optimizer (autograd)", dict(device_optimizer=True), False),
            ("+ device_optimizer (direct step)", dict(device_optimizer=True), True))
    lines = [f"{'pre-stage epoch':<14}{'batches':>8}" + "".join(f"{w[0] + ' ms':>38}" for w in ways) + "   per batch ms",
             "(%d epochs per call, median of %d calls, min .. max, per epoch; host clock to a device synchronise; calls alternating)" % (EPOCHS, EPOCH_WINDOWS)]
    for name, users, n_items, density, ratings, hidden, latent, batch in EPOCH_SHAPES:
        m = feed_matrix(users, n_items, density, ratings)

        def epochs_ms(kw, direct):
            torch.manual_seed(5)
            np.random.seed(6)
            vae = VAE(m.shape[1], hidden, latent).cuda()
            vae_hooks.DIRECT_STEP = direct
            try:
                with tempfile.TemporaryDirectory() as where, contextlib.redirect_stdout(io.StringIO()):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    train_variational_autoencoder(vae, m, m, EPOCHS, batch, 1e-3, "Recall@10", where, device_feed=True, sparse_input=True,
                                                  device_holdout=True, device_latent=True, device_decoder=True, **kw)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e3 / EPOCHS
            finally:
                vae_hooks.DIRECT_STEP = True

        for _, kw, direct in ways:   # warm-up: code objects, rocBLAS picks, the allocator's pools
            epochs_ms(kw, direct)
        t = {w[0]: [] for w in ways}
        for _ in range(EPOCH_WINDOWS):
            for tag, kw, direct in ways:
                t[tag].append(epochs_ms(kw, direct))
        batches = -(-m.shape[0] // batch)
        cell = lambda tag: f"{float(np.median(t[tag])):9.1f} ({min(t[tag]):.1f} .. {max(t[tag]):.1f})"
        per_batch = " / ".join(f"{float(np.median(t[w[0]])) / batches:.3f}" for w in ways)
        lines.append(f"{name:<14}{batches:>8}" + "".join(f"{cell(w[0]):>38}" for w in ways) + "   " + per_batch)
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "vae_optimizer_bench needs the GPU"
    text = "\n".join(optimizer_table(utility_engine()) + [""] + epoch_table()) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

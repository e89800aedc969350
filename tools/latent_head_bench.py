#!/usr/bin/env python3
"""The VAE encoder behind its first pre-activation in train mode (train_SDRM.py:244-250: tanh, the second Linear, chunk, the KL,
the reparameterisation; forward and backward) and one pre-stage epoch, one process, at the three EPOCH_SHAPES of
tools/input_layer_bench.py.

Part 1, forward + backward of that tail for one batch, HIP events, two ways:

  torch    what `VAE.encode_rows` runs behind `sparse_input_linear`: encoder[1:], chunk, the KL line, randn_like and the
           reparameterisation, then autograd to pre.grad, W2.grad and b2.grad for upstream gradients gz and gkl
  engine   sdrm_vae_latent_fwd (drawing on the device) + sdrm_vae_latent_bwd, and the two entry points on their own

Warm-up, then WINDOWS timed windows per variant, the variants alternating inside every round; the table gives the median window
and the min .. max spread in us per batch.  Before timing, the two ways are compared on one injected eps.

Part 2, `train_variational_autoencoder(device_feed=True, sparse_input=True, device_holdout=True)` for EPOCHS epochs without and
with `device_latent=True`: host clock around a call that ends in a device synchronise, calls alternating, ms per epoch (train half
+ evaluation half, checkpoint writes included in both).

`--out FILE` also writes the tables there (profiles/vae_latent_head_bench.txt is such a file)."""
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
from sdrm_amd.engine import utility_engine  # noqa: E402
from sdrm_amd.vae_hooks import VAE, train_variational_autoencoder  # noqa: E402
from encode_bench import window  # noqa: E402
from input_layer_bench import EPOCH_SHAPES, EPOCH_WINDOWS, EPOCHS, REPS, WARMUP, WINDOWS, feed_matrix  # noqa: E402

ANNEAL = 0.1


def head_table(eng):
    lines = [f"{'latent head, fwd + bwd':<24}{'H / L / b':>16}{'torch us':>26}{'engine us':>26}{'fwd us':>9}{'bwd us':>9}   fastest",
             "(median of %d windows of %d batches, min .. max; variants alternating)" % (WINDOWS, REPS)]
    for name, _, _, _, _, hidden, latent, batch in EPOCH_SHAPES:
        gen = torch.Generator("cuda").manual_seed(3)
        tail = torch.nn.Sequential(torch.nn.Tanh(), torch.nn.Linear(hidden, 2 * latent)).cuda()
        w2, b2 = tail[1].weight, tail[1].bias
        pre = torch.randn(batch, hidden, device="cuda", generator=gen).requires_grad_()
        gz = torch.randn(batch, latent, device="cuda", generator=gen) / batch
        gkl = torch.tensor(ANNEAL, device="cuda")
        rows = torch.randperm(20000, device="cuda", generator=gen)[:batch].contiguous()

        def torch_tail(eps=None):
            pre.grad = w2.grad = b2.grad = None
            h = tail(pre)
            mu, logvar = torch.chunk(h, chunks=2, dim=1)
            kl = -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1))
            e = torch.randn_like(mu) if eps is None else eps
            z = mu + 1 * e * torch.exp(0.5 * logvar)
            torch.autograd.backward([z, kl], [gz, gkl])
            return z, kl

        def v_fwd(eps=None):
            return eng.vae_latent_fwd(pre.detach(), w2.detach(), b2.detach(), rows=rows, seed=11, step=3, eps=eps)

        saved = v_fwd()[2]

        def v_bwd():
            return eng.vae_latent_bwd(saved, w2.detach(), gz, gkl)

        def v_engine():
            return eng.vae_latent_bwd(v_fwd()[2], w2.detach(), gz, gkl)

        # faster and different is not faster: with one injected eps the two ways compute the same values
        eps = torch.randn(batch, latent, device="cuda", generator=gen)
        z_t, kl_t = torch_tail(eps)
        z_e, kl_e, s_e = v_fwd(eps)
        got = (z_e, kl_e) + eng.vae_latent_bwd(s_e, w2.detach(), gz, gkl)
        for a, b in zip(got, (z_t.detach(), kl_t.detach(), pre.grad, w2.grad, b2.grad)):
            err = float((a.double() - b.double()).abs().max() / b.double().abs().max())
            assert err <= 1e-4, (name, err)
        variants = [("torch", torch_tail), ("engine", v_engine), ("fwd", v_fwd), ("bwd", v_bwd)]
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
        lines.append(f"{name:<24}{f'{hidden} / {latent} / {batch}':>16}{cell('torch'):>26}{cell('engine'):>26}{med['fwd']:>9.1f}{med['bwd']:>9.1f}   "
                     f"{'engine' if med['engine'] < med['torch'] else 'torch'}")
        print(lines[-1], flush=True)
    return lines


def epoch_table():
    lines = [f"{'pre-stage epoch':<18}{'batches':>8}{'feed + sparse + holdout ms':>32}{'+ device_latent ms':>28}   fastest",
             "(%d epochs per call, median of %d calls, min .. max, per epoch; host clock to a device synchronise; calls alternating)" % (EPOCHS, EPOCH_WINDOWS)]
    for name, users, n_items, density, ratings, hidden, latent, batch in EPOCH_SHAPES:
        m = feed_matrix(users, n_items, density, ratings)

        def epochs_ms(flag):
            torch.manual_seed(5)
            np.random.seed(6)
            vae = VAE(n_items, hidden, latent).cuda()
            with tempfile.TemporaryDirectory() as where, contextlib.redirect_stdout(io.StringIO()):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                train_variational_autoencoder(vae, m, m, EPOCHS, batch, 1e-3, "Recall@10", where, device_feed=True, sparse_input=True,
                                              device_holdout=True, device_latent=flag)
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
        lines.append(f"{name:<18}{-(-m.shape[0] // batch):>8}{cell(False):>32}{cell(True):>28}   {'device_latent' if med[True] < med[False] else 'without'}")
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "latent_head_bench needs the GPU"
    text = "\n".join(head_table(utility_engine()) + [""] + epoch_table()) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The VAE decoder and the multinomial loss in train mode (train_SDRM.py:252-254 and :141-142; forward and backward) and one
pre-stage epoch, one process, at the three EPOCH_SHAPES of tools/input_layer_bench.py.

Part 1, forward + backward of decoder + loss for one batch, HIP events, two ways:

  torch    what the train half runs with `device_feed=True`: `model.decode(z)` + `multinomial_nll` (csrc/nll.h), then autograd to
           z.grad and the four parameters' gradients
  engine   sdrm_vae_decoder_nll_fwd + sdrm_vae_decoder_nll_bwd, and the two entry points on their own

Warm-up, then WINDOWS timed windows per variant, the variants alternating inside every round; the table gives the median window
and the min .. max spread in us per batch.  Before timing, the two ways are compared on one batch at 1e-4.

Part 2, `train_variational_autoencoder(device_feed=True, sparse_input=True, device_holdout=True, device_latent=True)` for EPOCHS
epochs without and with `device_decoder=True`: host clock around a call that ends in a device synchronise, calls alternating, ms per
epoch (train half + evaluation half, checkpoint writes included in both).

`--out FILE` also writes the tables there (profiles/vae_decoder_head_bench.txt is such a file)."""
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
from sdrm_amd.vae_hooks import VAE, multinomial_nll, train_variational_autoencoder  # noqa: E402
from encode_bench import window  # noqa: E402
from input_layer_bench import EPOCH_SHAPES, EPOCH_WINDOWS, EPOCHS, REPS, WARMUP, WINDOWS, feed_matrix  # noqa: E402


def head_table(eng):
    lines = [f"{'decoder head, fwd + bwd':<24}{'L / H / I / b':>24}{'torch us':>28}{'engine us':>28}{'fwd us':>9}{'bwd us':>9}   fastest",
             "(median of %d windows of %d batches, min .. max; variants alternating)" % (WINDOWS, REPS)]
    for name, users, n_items, density, ratings, hidden, latent, batch in EPOCH_SHAPES:
        m = feed_matrix(users, n_items, density, ratings)
        n_items = m.shape[1]
        csr = eng.csr_to_device(m)
        gen = torch.Generator("cuda").manual_seed(3)
        torch.manual_seed(4)
        model = VAE(n_items, hidden, latent).cuda()
        params = [model.decoder[0].weight, model.decoder[0].bias, model.decoder[2].weight, model.decoder[2].bias]
        z = torch.randn(batch, latent, device="cuda", generator=gen).requires_grad_()
        rows = torch.randperm(m.shape[0], device="cuda", generator=gen)[:batch].contiguous()
        tensors = [z.detach()] + [p.detach() for p in params]
        scale = torch.ones((), device="cuda")

        def torch_head():
            z.grad = None
            for p in params:
                p.grad = None
            loss = multinomial_nll(model.decode(z), csr, rows=rows)
            loss.backward()
            return loss

        def v_fwd():
            return eng.vae_decoder_nll_fwd(*tensors, csr, rows=rows, check=False)

        saved = v_fwd()[1]

        def v_bwd():
            return eng.vae_decoder_nll_bwd(saved, *tensors, csr, rows=rows, scale=scale)

        def v_engine():
            return eng.vae_decoder_nll_bwd(v_fwd()[1], *tensors, csr, rows=rows, scale=scale)

        # faster and different is not faster: the two ways compute the same values
        loss_t = torch_head()
        loss_e, s_e = v_fwd()
        got = (loss_e,) + eng.vae_decoder_nll_bwd(s_e, *tensors, csr, rows=rows, scale=scale)
        for a, b in zip(got, [loss_t.detach(), z.grad] + [p.grad for p in params]):
            err = float((a.double() - b.double()).abs().max() / b.double().abs().max())
            assert err <= 1e-4, (name, err)
        variants = [("torch", torch_head), ("engine", v_engine), ("fwd", v_fwd), ("bwd", v_bwd)]
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
        lines.append(f"{name:<24}{f'{latent} / {hidden} / {n_items} / {batch}':>24}{cell('torch'):>28}{cell('engine'):>28}{med['fwd']:>9.1f}"
                     f"{med['bwd']:>9.1f}   {'engine' if med['engine'] < med['torch'] else 'torch'}")
        print(lines[-1], flush=True)
    return lines


def epoch_table():
    lines = [f"{'pre-stage epoch':<18}{'batches':>8}{'feed + sparse + holdout + latent ms':>40}{'+ device_decoder ms':>28}   fastest",
             "(%d epochs per call, median of %d calls, min .. max, per epoch; host clock to a device synchronise; calls alternating)" % (EPOCHS, EPOCH_WINDOWS)]
    for name, users, n_items, density, ratings, hidden, latent, batch in EPOCH_SHAPES:
        m = feed_matrix(users, n_items, density, ratings)

        def epochs_ms(flag):
            torch.manual_seed(5)
            np.random.seed(6)
            vae = VAE(m.shape[1], hidden, latent).cuda()
            with tempfile.TemporaryDirectory() as where, contextlib.redirect_stdout(io.StringIO()):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                train_variational_autoencoder(vae, m, m, EPOCHS, batch, 1e-3, "Recall@10", where, device_feed=True, sparse_input=True,
                                              device_holdout=True, device_latent=True, device_decoder=flag)
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
        lines.append(f"{name:<18}{-(-m.shape[0] // batch):>8}{cell(False):>40}{cell(True):>28}   {'device_decoder' if med[True] < med[False] else 'without'}")
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "decoder_head_bench needs the GPU"
    text = "\n".join(head_table(utility_engine()) + [""] + epoch_table()) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

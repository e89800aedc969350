#!/usr/bin/env python3
"""The evaluation half of a MultiVAE++ pre-stage epoch, the torch forward against `Engine.vae_eval_holdout` (csrc/eval_half.h), one
process, at the three EPOCH_SHAPES of tools/nll_bench.py (the same synthetic feeds, the same seeds).

Before any timing, per shape: one evaluation done the two ways from equal weights - the engine's logits against the torch forward's at
the decode bar (1e-4 normwise), the largest element difference tau, and the users decided at 2 tau (no other unmasked score within 2 tau
of a held item's) compared bit for bit, with the count of the undecided.  With untrained weights and thousands of items most users are
undecided, so two more figures cover all users: how many users' metrics differ between the two ways in all, and how many of the
engine's scores differ from `Engine.rank_metrics` on the engine's OWN logits (none may: with the logits at the bar, that holds the
ranking of every user to the parent's ranking kernel bit for bit, decided or not).

Part 1, the evaluation half alone: `evaluate_holdout` with `device_forward` off and on, the split included in both.  Device time by HIP
events (REPS calls per window) and wall time of one call to a device synchronise; WINDOWS windows per variant, the variants
alternating inside every round; median with min .. max.  With it the launches of one engine call by `sdrm_launch_count`, and the
staging made once per call against once per batch (the same call with `batch` users per call, i.e. one engine call per batch).

Part 2, one epoch: `train_variational_autoencoder` with the six flags, without and with `device_eval=True`, under the epoch protocol
of nll_bench (host clock around a call that ends in a device synchronise, calls alternating, ms per epoch, checkpoint writes included).

`--out FILE` also writes the tables there (profiles/eval_half_bench.txt is such a file)."""
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
from sdrm_amd.vae_hooks import VAE, evaluate_holdout, train_variational_autoencoder  # noqa: E402
from encode_bench import window  # noqa: E402
from nll_bench import EPOCH_SHAPES, EPOCH_WINDOWS, EPOCHS, WINDOWS, feed  # noqa: E402

REPS, WARMUP, BATCH, K = 10, 3, 500, 10
FAILED = []   # shapes whose two evaluations did not agree at the bars (reported after the tables are written)
SIX = dict(device_feed=True, sparse_input=True, device_holdout=True, device_latent=True, device_decoder=True, device_optimizer=True)


def weights(vae):
    mods = (vae.encoder[0], vae.encoder[2], vae.decoder[0], vae.decoder[2])
    return tuple(t.detach() for mod in mods for t in (mod.weight, mod.bias))


def compare(eng, vae, csr, n, n_items):
    """One evaluation the two ways: (normwise error, tau, max|s|, users with held items, undecided, decided users that differ, equal nan
    pattern, users that differ in all, users whose score is not `rank_metrics` of the engine's own logits)."""
    train, held = eng.holdout_split(csr, seed=7, draw=1)
    vae.eval()
    vae.is_training = 0
    with torch.no_grad():
        ref = torch.cat([vae(eng.csr_rows_to_dense(train, row0=lo, b=min(BATCH, n - lo)))[0] for lo in range(0, n, BATCH)])
    got = torch.empty(n, n_items, dtype=torch.float32, device=eng.device)
    s_eng = eng.vae_eval_holdout(*weights(vae), train, held, K, 0, batch=BATCH, logits=got, check=True)
    s_ref = torch.cat([eng.rank_metrics(ref[lo:lo + BATCH], held, train=train, ks=(K,), row0=lo)[0][0] for lo in range(0, n, BATCH)])
    s_own = torch.cat([eng.rank_metrics(got[lo:lo + BATCH], held, train=train, ks=(K,), row0=lo)[0][0] for lo in range(0, n, BATCH)])
    own_differ = int(((s_eng != s_own) & ~(torch.isnan(s_eng) & torch.isnan(s_own))).sum())
    err = float(torch.linalg.norm(got.double() - ref.double()) / torch.linalg.norm(ref.double()))
    tau = float((got.double() - ref.double()).abs().max())
    # decided at 2 tau, on the device: per user the smallest gap between a held item and any other unmasked item
    masked = ref.double().clone()
    tp, ti = train[0], train[1]
    rows_t = torch.repeat_interleave(torch.arange(n, device=eng.device), tp[1:] - tp[:-1])
    masked[rows_t, ti[:int(tp[-1])].long()] = float("-inf")
    hp, hi = held[0], held[1]
    rows_h = torch.repeat_interleave(torch.arange(n, device=eng.device), hp[1:] - hp[:-1])
    cols_h = hi[:int(hp[-1])].long()
    undecided = torch.zeros(n, dtype=torch.bool, device=eng.device)
    for lo in range(0, rows_h.numel(), 4096):
        r, c = rows_h[lo:lo + 4096], cols_h[lo:lo + 4096]
        gap = (masked[r] - masked[r, c][:, None]).abs()
        gap[torch.arange(r.numel(), device=eng.device), c] = float("inf")
        undecided[r[(gap <= 2 * tau).any(dim=1)]] = True
    with_held = (hp[1:] - hp[:-1]) > 0
    dec = with_held & ~undecided
    differ = int((s_eng[dec] != s_ref[dec]).sum())
    same_nan = bool((torch.isnan(s_eng) == torch.isnan(s_ref)).all())
    differ_all = int((s_eng[with_held] != s_ref[with_held]).sum())
    return err, tau, float(ref.abs().max()), int(with_held.sum()), int((with_held & undecided).sum()), differ, same_nan, differ_all, own_differ


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def eval_table(eng):
    head = [f"{'equal weights':<14}{'logits, normwise':>18}{'tau':>11}{'tau / max|s|':>14}{'with held':>11}{'undecided':>11}{'decided, differ':>17}{'nan pattern':>13}{'differ in all':>15}"
            f"{'not rank_metrics of own logits':>32}"]
    lines = [f"{'evaluation half':<14}{'batches':>8}{'torch, device ms':>26}{'engine, device ms':>26}{'torch, wall ms':>26}{'engine, wall ms':>26}"
             f"{'launches':>10}{'staged per batch, device ms':>30}",
             "(evaluate_holdout with device_forward off / on, the split included; median of %d windows, min .. max; device: HIP events, %d calls "
             "per window; wall: one call to a device synchronise; variants alternating; launches: one engine call, by sdrm_launch_count; "
             "staged per batch: one engine call per batch of %d users)" % (WINDOWS, REPS, BATCH)]
    for name, users, n_items, density, ratings, hidden, latent, _ in EPOCH_SHAPES:
        m = feed(users, n_items, density, ratings)
        n = m.shape[0]
        csr = eng.csr_to_device(m)
        torch.manual_seed(5)
        vae = VAE(n_items, hidden, latent).cuda()
        err, tau, smax, held_users, undecided, differ, same_nan, differ_all, own_differ = compare(eng, vae, csr, n, n_items)
        if not (err <= 1e-4 and differ == 0 and same_nan and own_differ == 0):
            FAILED.append(name)
        head.append(f"{name:<14}{err:>18.2e}{tau:>11.2e}{tau / smax:>14.2e}{held_users:>11}{undecided:>11}{differ:>17}{'equal' if same_nan else 'DIFFERS':>13}"
                    f"{differ_all:>15}{own_differ:>32}")
        print(head[-1], flush=True)
        train, held = eng.holdout_split(csr, seed=7, draw=1)
        w = weights(vae)
        scores = torch.empty(n, dtype=torch.float64, device=eng.device)

        def v_torch():
            return evaluate_holdout(vae, eng, csr, 7, 1, "Recall@10")

        def v_engine():
            return evaluate_holdout(vae, eng, csr, 7, 1, "Recall@10", device_forward=True)

        def v_per_batch():   # the same launches with the staging made for every batch: one call per batch, on that batch's rows of the two CSRs
            eng.holdout_split(csr, seed=7, draw=1, check=False)
            for lo in range(0, n, BATCH):
                b = min(BATCH, n - lo)
                tr = (train[0][lo:lo + b + 1].contiguous(), train[1], None, (b, n_items))
                he = (held[0][lo:lo + b + 1].contiguous(), held[1], None, (b, n_items))
                eng.vae_eval_holdout(*w, tr, he, K, 0, batch=BATCH, out=scores[lo:lo + b])
        before = eng.launch_count()
        eng.vae_eval_holdout(*w, train, held, K, 0, batch=BATCH)
        launches = eng.launch_count() - before
        variants = {"torch": v_torch, "engine": v_engine, "per_batch": v_per_batch}
        for fn in variants.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        dev = {tag: [] for tag in variants}
        host = {tag: [] for tag in variants}
        for _ in range(WINDOWS):
            for tag, fn in variants.items():
                dev[tag].append(window(fn, REPS) / 1e3)
            for tag, fn in variants.items():
                host[tag].append(wall(fn))
        eng.feed_status()
        cell = lambda t, tag: f"{float(np.median(t[tag])):9.3f} ({min(t[tag]):.3f} .. {max(t[tag]):.3f})"
        lines.append(f"{name:<14}{-(-n // BATCH):>8}{cell(dev, 'torch'):>26}{cell(dev, 'engine'):>26}{cell(host, 'torch'):>26}{cell(host, 'engine'):>26}"
                     f"{launches:>10}{cell(dev, 'per_batch'):>30}")
        print(lines[-1], flush=True)
    return head + [""] + lines


def epoch_table():
    lines = [f"{'pre-stage epoch':<14}{'batches':>8}{'six flags ms':>28}{'+ device_eval ms':>28}   fastest",
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
                train_variational_autoencoder(vae, m, m, EPOCHS, batch, 1e-3, "Recall@10", where, device_eval=flag, **SIX)
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
        lines.append(f"{name:<14}{-(-m.shape[0] // batch):>8}{cell(False):>28}{cell(True):>28}   {'device_eval' if med[True] < med[False] else 'six flags'}")
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "eval_half_bench needs the GPU"
    text = "\n".join(eval_table(utility_engine()) + [""] + epoch_table()) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    if FAILED:
        sys.exit("the two evaluations differ beyond the bars at: " + ", ".join(FAILED))


if __name__ == "__main__":
    main()

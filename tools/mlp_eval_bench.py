#!/usr/bin/env python3
"""The evaluation half of an epoch of the MLP evaluator, two ways, at the three shapes of tools/mlp_train_bench.py (widths 512 / 256 / 256;
rows x items): the ML-100k fixture 843 x 1008, the ML-1M shape 6040 x 3706 at 4.5 %, the ADM shape 5541 x 3568 at 0.35 %.  The held rows
are the last rows - floor(0.8 rows) rows, as `mlp_eval.compute_mlp_results` splits them.  Timed, each REPS times with the spread shown
(host clock around work that ends in a device synchronise):

  (a) the validation pass: device = ONE `Engine.mlp_eval(row0=n_fit, out=False, sse=True)` on the resident CSR and the read-back of its
      scalar (csrc/mlp_eval.h); torch = the driver's `validation_rmse` on the same GPU - the only reference that can run: the held rows
      densified on the host, uploaded in chunks of 256, the module's forward.  And the predict: device = one `Engine.mlp_eval` that
      writes the held rows' probabilities; torch = `MLP.predict` over the same chunks, concatenated.
  (b) a whole epoch with `device_train=True` - one `Engine.mlp_train_steps` call over a shuffled order of the train rows - followed by
      the validation pass, device against torch.
  (c) k_mlp_fold alone, two events around the launch, against the bytes it has to move (W1 read once, D written: 1.125 |W1|, and the
      partial B_f) at 6.3 TB/s.

`--out FILE` appends the table to FILE (profiles/mlp_eval_bench.txt is such a file)."""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from mlp_train_bench import BATCH, HBM, SHAPES, matrix  # noqa: E402
from sdrm_amd import mlp_eval  # noqa: E402
from sdrm_amd.engine import utility_engine  # noqa: E402

H1 = mlp_eval.WIDTHS[0]
REPS = 5
FOLD_ITEMS = 16   # csrc/mlp_train.h: MLP_W1_ITEMS


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(ms):
    return f"{np.median(ms):.2f} ({min(ms):.2f} .. {max(ms):.2f})"


def beyond(a, b):
    """Whether two sets of repeats differ beyond their run-to-run spread: the gap between them against the wider of the two spreads."""
    lo, hi = (a, b) if np.median(a) < np.median(b) else (b, a)
    return min(hi) - max(lo) > max(max(a) - min(a), max(b) - min(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mlp_eval_bench needs the GPU"
    eng = utility_engine()
    head = f"{'ms: median (min .. max)':<34}{'rows':>6}{'items':>7}{'held':>6}"
    lines = []
    for name in args.shapes:
        train = matrix(name)
        n_rows, n_items = train.shape
        n_fit = int(math.floor(0.8 * n_rows))
        held = train[n_fit:]
        rng = np.random.default_rng(1)
        torch.manual_seed(0)
        model = mlp_eval.MLP(n_rows, n_items).cuda()
        live = [p.data for p in model.engine_weights()]
        m, v = [torch.zeros_like(t) for t in live], [torch.zeros_like(t) for t in live]
        csr_dev = eng.csr_to_device(train)
        state = {"step0": 0, "call": 0}
        steps = -(-n_fit // BATCH)

        def dev_val():
            return float(eng.mlp_eval(live, csr_dev, row0=n_fit, out=False, sse=True, check=False).item())

        def torch_val():
            model.eval()
            return mlp_eval.validation_rmse(model, held, "cuda")

        def dev_predict():
            return eng.mlp_eval(live, csr_dev, row0=n_fit, check=False)

        def torch_predict():
            model.eval()
            return torch.cat([model.predict(mlp_eval._dense(held[s:s + mlp_eval.PREDICT_BATCH], "cuda"))
                              for s in range(0, held.shape[0], mlp_eval.PREDICT_BATCH)])

        def train_epoch():
            rows = torch.from_numpy(rng.permutation(n_fit).astype(np.int64)).cuda()
            eng.mlp_train_steps(live, m, v, csr_dev, rows, BATCH, state["step0"], seed=0, call_id=state["call"], check=False)
            state["step0"] += steps
            state["call"] += 1

        # the two paths agree before anything is timed
        rmse_d, rmse_t = math.sqrt(dev_val() / (held.shape[0] * n_items)), torch_val()
        worst = float((dev_predict() - torch_predict()).abs().max())
        assert abs(rmse_d - rmse_t) <= 1e-6 * rmse_t and worst <= 1e-5, (rmse_d, rmse_t, worst)
        t = {}
        for key, fn in (("val device", dev_val), ("val torch", torch_val), ("predict device", dev_predict), ("predict torch", torch_predict)):
            host_ms(fn)                                                # warm-up: code objects, scratch
            t[key] = [host_ms(fn) for _ in range(REPS)]
        host_ms(train_epoch)
        for key, val in (("epoch device eval", dev_val), ("epoch torch eval", torch_val)):
            t[key] = [host_ms(lambda: (train_epoch(), val())) for _ in range(REPS)]
        eng.feed_status()
        # (c) the fold alone
        fold_class = next(k for k in (eng.lib.sdrm_profile_name(c).decode() for c in range(eng.lib.sdrm_profile_classes())) if "k_mlp_fold" in k)
        eng.profile_begin(capacity=64, only=fold_class)
        for _ in range(REPS + 1):
            dev_val()
        torch.cuda.synchronize()
        fold_ms, fold_n, _ = eng.profile_end()[fold_class]
        w1 = 8 * n_items * H1 * 4
        fold_bytes = w1 + w1 // 8 + -(-n_items // FOLD_ITEMS) * 8 * H1 * 8
        fold_us = fold_ms / fold_n * 1e3

        def row(what, a, b):
            return (f"{name + ', ' + what:<34}{n_rows:>6}{n_items:>7}{held.shape[0]:>6}   device {spread(t[a]):>26}   torch {spread(t[b]):>30}   torch / device "
                    f"{np.median(t[b]) / np.median(t[a]):>6.1f}x   beyond the spread: {'yes' if beyond(t[a], t[b]) else 'NO'}")
        lines += [row("validation pass", "val device", "val torch"), row("predict", "predict device", "predict torch"),
                  row("epoch: train + validation", "epoch device eval", "epoch torch eval"),
                  f"{name + ', k_mlp_fold':<34}{fold_us:.1f} us per launch under the event profile ({fold_n} launches), {fold_bytes / 1e6:.1f} MB = "
                  f"{fold_bytes / (fold_us * 1e-6) / HBM:.1%} of 6.3 TB/s; validation RMSE device {rmse_d:.9f} torch {rmse_t:.9f}, worst "
                  f"difference of a probability {worst:.1e}", ""]
        for ln in lines[-5:]:
            print(ln, flush=True)
        del model, live, m, v
        torch.cuda.empty_cache()
    text = "\n".join([head] + lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()

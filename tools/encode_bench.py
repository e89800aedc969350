#!/usr/bin/env python3
"""The frozen VAE encode hook (train_SDRM.py:323) at the BASELINE shapes, three ways, one process, HIP events:

  module   sdrm_csr_rows_to_dense + the PyTorch module's `encode` on the dense batch (the path without `engine_encode`)
  dense    sdrm_csr_rows_to_dense + sdrm_vae_encode
  csr      sdrm_vae_encode_csr (no dense batch)

Each batch is `rows` = a slice of a permutation of the resident CSR feed, as pipeline.DeviceFeed issues it; every variant
returns z only (kl null), as train_SDRM uses it.  Warm-up, then WINDOWS timed windows per variant, the variants alternating
inside every round so that drift hits all three; the table gives the median window and the min .. max spread in us per call.
`--out FILE` also writes the table there (profiles/vae_encode_bench.txt is such a file)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrm_amd import synth  # noqa: E402
from sdrm_amd.engine import Engine  # noqa: E402
from sdrm_amd.train_SDRM import VAE  # noqa: E402

# name, feed rows, n_items, density (None: the real ML-100k rows), ratings, hidden, latent, batch
SHAPES = [
    ("ML-100k B=550", 843, 1008, None, True, 930, 830, 550),
    ("ML-1M B=160", 6034, 3125, 0.05, True, 600, 340, 160),
    ("ML-1M B=8192", 8192, 3125, 0.05, True, 600, 340, 8192),
    ("ADM B=850", 10621, 8582, 0.012, False, 200, 40, 850),
]
WINDOWS, WARMUP = 7, 5


def ml100k_rows():
    from scipy.sparse import csr_matrix
    z = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ml100k.npz"))
    return csr_matrix((z["train_test_data"].astype(np.float32), z["train_test_indices"].astype(np.int32),
                       z["train_test_indptr"].astype(np.int64)), shape=tuple(int(v) for v in z["train_test_shape"]))


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "encode_bench needs the GPU"
    e = Engine(8, 8, 4, 0, 16)
    lines = [f"{'shape':<15}{'nnz/row':>8}{'module us':>22}{'dense us':>22}{'csr us':>22}   fastest",
             "(median of %d windows, min .. max; one process, variants alternating; z only)" % WINDOWS]
    for name, n_rows, n_items, density, ratings, hidden, latent, batch in SHAPES:
        m = ml100k_rows() if density is None else synth.synth_feed_csr(n_rows, n_items, density, seed=7, ratings=ratings)
        tensors = synth.synth_vae_encoder(n_items, hidden, latent, seed=8)
        csr = e.csr_to_device(m)
        e.vae_encoder_load(*tensors)
        vae = VAE(n_items, hidden, latent).cuda().eval()
        with torch.no_grad():
            for p, t in zip((vae.encoder[0].weight, vae.encoder[0].bias, vae.encoder[2].weight, vae.encoder[2].bias), tensors):
                p.copy_(torch.from_numpy(t))
        rows = torch.from_numpy(np.random.RandomState(9).permutation(m.shape[0])[:batch].astype(np.int64)).cuda()

        def v_module():
            with torch.no_grad():
                return vae.encode(e.csr_rows_to_dense(csr, rows=rows, check=False))[0]

        def v_dense():
            return e.vae_encode(e.csr_rows_to_dense(csr, rows=rows, check=False))

        def v_csr():
            return e.vae_encode_csr(csr, rows=rows, check=False)
        variants = [("module", v_module), ("dense", v_dense), ("csr", v_csr)]
        ref = v_module().double()
        for tag, fn in variants[1:]:   # faster and different is not faster
            err = float((fn().double() - ref).abs().max() / ref.abs().max())
            assert err <= 1e-4, (name, tag, err)
        for _, fn in variants:
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        reps = 30 if batch >= 4096 else 200
        t = {tag: [] for tag, _ in variants}
        for _ in range(WINDOWS):
            for tag, fn in variants:
                t[tag].append(window(fn, reps))
        e.feed_status()
        med = {tag: float(np.median(v)) for tag, v in t.items()}
        cell = lambda tag: f"{med[tag]:8.1f} ({min(t[tag]):.1f} .. {max(t[tag]):.1f})"
        lines.append(f"{name:<15}{m.nnz / m.shape[0]:>8.0f}{cell('module'):>22}{cell('dense'):>22}{cell('csr'):>22}   {min(med, key=med.get)}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    e.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/vae_encode.npz from the upstream reference (CPU, where the reference exists; see make_golden.py).

The reference's own `VAE(...).eval().encode` (train_SDRM.py:241-250, is_training == 0) with injected `synth_vae_encoder`
tensors, on the inputs tests/vae_encode_ref.py::case_inputs makes for each row of its CASES table.  Stored per case: the
dims / seeds the inputs are rebuilt from, z and kl.  The inputs themselves are not stored: the real rows are rows of
tests/golden/ml100k.npz, the others are drawn from a seed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_vae_encode_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import load_reference  # noqa: E402
import torch  # noqa: E402
import vae_encode_ref as ver  # noqa: E402


def main():
    ref = load_reference()
    out = {"n_cases": np.asarray(len(ver.CASES))}
    for i, (kind, n_items, hidden, latent, n, density, ratings, empty_row) in enumerate(ver.CASES):
        (w1, b1, w2, b2), m = ver.case_inputs(i)
        vae = ref.VAE(n_items, hidden, latent).eval()
        assert vae.is_training == 0
        with torch.no_grad():
            vae.encoder[0].weight.copy_(torch.from_numpy(w1)); vae.encoder[0].bias.copy_(torch.from_numpy(b1))
            vae.encoder[2].weight.copy_(torch.from_numpy(w2)); vae.encoder[2].bias.copy_(torch.from_numpy(b2))
            z, kl = vae.encode(torch.from_numpy(m.toarray().astype(np.float32)))
        out[f"c{i}_dims"] = np.asarray([n_items, hidden, latent, n, 400 + i, 500 + i, int(kind == "ml100k"), int(round(density * 1e6)),
                                        ratings, empty_row])
        out[f"c{i}_nnz"] = np.asarray(m.nnz)
        out[f"c{i}_z"] = z.numpy().astype(np.float32)
        out[f"c{i}_kl"] = np.asarray(kl.item(), dtype=np.float32)
    path = os.path.join(HERE, "vae_encode.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

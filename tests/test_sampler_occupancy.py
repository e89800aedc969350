"""PHILOX full-resolution sampling at the edges of the 32x32x32 tile (csrc/gemm.h), whose K loop waits for its operand loads by count
and whose waves outside the matrix end their own loop with the wait for theirs (tests/test_sampler_kernel_resources.py holds the
generated code).  Written for the builds that raised the tile's residency to eight work-groups per CU - measured and dropped,
profiles/sampler_occupancy.txt - and kept for the kernels as they are.  The smallest shapes that reach the edges:

  * L = W = 340, T = 78, H = 1 (the headline net): the last K-step of every layer holds 20 real k of 32;
    L = W = 136, T = 12, H = 2: 8 of 32;
  * n = 33, 64, 95 rows: a last row tile with one row, a full one, and one row short of full;
  * the reverse update as its own kernel (fused = 0), in the out layer's epilogue by the size rule (1) and always (2);
  * one row chain - these calls then run in the persistent kernel (csrc/sample_persist.h), which holds the tile body of both layer
    kinds, or, with that switched off, as one launch per layer - and two chains forced (chains are whole 64-row granules: 95 rows run
    as 64 + 31, the smaller calls stay one chain);
  * the call driven one reverse step at a time and in one piece.

Every call is held to the CPU oracle, fed the same randoms by oracle/philox_ref.py, at the bar tests/test_hip_parity.py sets for
sampling (1e-4, normwise and in the largest element).  Rows are independent through the reverse loop and the generator is keyed by
row, and at these sizes every chain runs on the same tile with the same fusion: for one value of `fused`, chain counts, launch forms and
step chunks all give the same bits.  Needs a real MI355X: `pytest -m gpu`."""
import itertools
import math

import numpy as np
import pytest
import torch

from sdrm_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-4      # tests/test_hip_parity.py: TOL, close()
ND = 0.9
SEED, CALL_ID, ROW0 = 77, 4, 1000
N_MAX = 95
DIMS = [(340, 340, 78, 1), (136, 136, 12, 2)]
ROWS = [33, 64, N_MAX]


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def rel_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.fixture(scope="module")
def oracle_latents():
    """dims -> (flat parameters, the oracle's latents of rows ROW0 .. ROW0 + N_MAX - 1): the generator is keyed by (row, column, step),
    so a call of n rows from ROW0 draws what the first n rows of the largest call draw - one oracle run per net serves every row count."""
    from oracle import philox_ref as pr
    from oracle import sdrm_oracle as orc
    out = {}
    for dims in DIMS:
        L, W, T, H = dims
        init = synth.init_params(L, W, T, H, seed=23)
        xT, z, keep, _ = pr.sample_randoms(SEED, CALL_ID, ROW0, N_MAX, L, T, ND, False)
        ref = orc.Oracle(L, W, T, H, init).sample(xT, z, keep).numpy()
        out[dims] = (synth.flatten_params(init, H), ref)
    return out


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "x".join(map(str, d)))
def test_sampling_at_the_tile_edges(engine_cls, oracle_latents, dims, n):
    L, W, T, H = dims
    flat, ref = oracle_latents[dims]
    ref = ref[:n]
    e = engine_cls(L, W, T, H, n)
    e.set_params(flat)
    for fused in (0, 1, 2):
        first = None
        # (persist, chains): the call in one persistent launch per sample_steps (one chain, fused), one launch per layer, two chains
        for (persist, chains), chunk in itertools.product(((1, 1), (0, 1), (1, 2)), (T, 1)):
            e.debug_set(fused_reverse=fused, chains=chains, sample_persist=persist)
            e.sample_begin(n, nd=ND, seed=SEED, call_id=CALL_ID, row0=ROW0)
            while e.sample_steps(chunk) > 0:
                pass
            out = e.sample_end().cpu()
            # a chain is a whole number of 64-row granules (csrc/sdrm_hip.hip: sdrm_sample_begin), so two chains forced are two from 65 rows on
            granted = math.ceil(n / (64 * math.ceil(math.ceil(n / chains) / 64)))
            assert e.sampler_chains == granted, (n, chains, e.sampler_chains)
            want_path = "persist" if (persist and granted == 1 and fused) else "per_layer"
            assert e.last_plan().sample_path == want_path, (fused, persist, chains, e.last_plan())
            got = out.numpy()
            print(dims, n, "fused", fused, "persist", persist, "chains", chains, "chunk", chunk, "rel_l2 %.2e rel_max %.2e" % (rel_l2(got, ref), rel_max(got, ref)))
            assert rel_l2(got, ref) <= TOL and rel_max(got, ref) <= TOL, (fused, persist, chains, chunk, rel_l2(got, ref), rel_max(got, ref))
            if first is None:
                first = out
            assert torch.equal(out, first), (fused, persist, chains, chunk, float((out - first).abs().max()))
    e.close()

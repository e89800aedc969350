"""One engine, every utility entry point that owns library scratch, at changing sizes: no call may touch what another one left.

The engine keeps the device scratch of these entry points in one pool of grow-only slots.  Two families landing on one slot would not
show in any family's own tests, so this test interleaves them all between a `vae_encoder_load` and its `vae_encode_csr`, and between an
`equal_sparsity_csr_begin` and its `_end` - the two things the C header promises to keep across other calls - at b = 33, then b = 300
(every slot regrows), then b = 33 again, and holds every result to the bits."""
import numpy as np
import pytest
import torch

import neumf_ref as nr
import vae_input_layer_ref as ilr
from sdrm_amd.engine import Engine

ITEMS, HIDDEN, LATENT = 70, 36, 12   # no extent on a multiple of 4 or 32
SEED, STEP, P_DROP = 0xC0FFEE, 3, 0.5
FACTOR, NEUMF_USERS = 8, 310


def _bytes(x):
    """Every tensor / array of a (nested) result as bytes; a CSR-shaped tuple only up to its entry count (the arrays may be longer)."""
    if x is None:
        return [b""]
    if isinstance(x, torch.Tensor):
        return [x.detach().cpu().contiguous().numpy().tobytes()]
    if isinstance(x, np.ndarray):
        return [np.ascontiguousarray(x).tobytes()]
    if isinstance(x, (tuple, list)):
        if len(x) == 4 and isinstance(x[0], torch.Tensor) and x[0].dtype == torch.int64 and isinstance(x[1], torch.Tensor) and x[1].dtype == torch.int32:
            ptr = x[0].cpu()
            lo, hi = int(ptr[0]), int(ptr[-1])
            return _bytes(ptr) + _bytes(x[1][lo:hi]) + _bytes(None if x[2] is None else x[2][lo:hi]) + [repr(tuple(int(v) for v in x[3])).encode()]
        return [b for y in x for b in _bytes(y)]
    return [repr(x).encode()]


def _inputs(device):
    rng = np.random.default_rng(20261)
    t = lambda *shape: torch.from_numpy((rng.standard_normal(shape) * 0.2).astype(np.float32)).to(device)
    vae = dict(w1=t(HIDDEN, ITEMS), b1=t(HIDDEN), w2=t(2 * LATENT, HIDDEN), b2=t(2 * LATENT), w3=t(HIDDEN, LATENT), b3=t(HIDDEN), w4=t(ITEMS, HIDDEN),
               b4=t(ITEMS))
    raw = torch.from_numpy(rng.random((33, ITEMS), dtype=np.float32)).to(device)
    neumf = [torch.from_numpy(v).to(device) for v in nr.weights(FACTOR, NEUMF_USERS, ITEMS, 99).values()]
    return vae, raw, neumf, ilr.case_feed(ITEMS, "ones", SEED, STEP, P_DROP), rng


def _round(e, v, neumf, feed, b):
    """One small call of every family at batch / row count b; everything they return."""
    sub = feed[:b]
    csr, csc = e.csr_to_device(sub), e.csc_to_device(sub)
    g = torch.Generator().manual_seed(b)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(e.device)
    out = [e.vae_decode(rnd(b, LATENT), v["w3"], v["b3"], v["w4"], v["b4"])]
    pre, rowscale = e.vae_input_layer_fwd(v["w1"], v["b1"], csr, row0=0, b=b, seed=SEED, step=STEP, p_drop=P_DROP)
    out += [pre, rowscale, e.vae_input_layer_wgrad(rnd(b, HIDDEN), rowscale, csc, lo=0, b=b, seed=SEED, step=STEP, p_drop=P_DROP)]
    z, kl, saved = e.vae_latent_fwd(pre, v["w2"], v["b2"], row0=0, seed=SEED, step=STEP)
    out += [z, kl, saved, e.vae_latent_bwd(saved, v["w2"], rnd(b, LATENT), rnd(1))]
    loss, dsaved = e.vae_decoder_nll_fwd(z, v["w3"], v["b3"], v["w4"], v["b4"], csr, row0=0, b=b)
    out += [loss, dsaved, e.vae_decoder_nll_bwd(dsaved, z, v["w3"], v["b3"], v["w4"], v["b4"], csr, row0=0, b=b)]
    train, held = e.holdout_split(csr, test_prop=0.2, seed=5, draw=1)
    out += [train, held, e.vae_eval_holdout(*(v[k] for k in ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")), train, held, 5, "ndcg", batch=max(1, b // 2))]
    out += [e.csr_transpose(csr), e.csr_vstack([csr, train])]
    comps, sigma = e.svd_fit(csr, csc, n_components=4, n_iter=2, seed=7, draw=0)
    out += [comps, sigma, e.svd_scores(csr, comps, row0=0, b=b)]
    users = torch.arange(b, dtype=torch.int32, device=e.device)
    items = (users * 7) % ITEMS
    out += [e.neumf_scores(neumf, users), e.neumf_pair_logits(neumf, users, items, labels=(users % 2).float())]
    return _bytes(out)


@pytest.mark.gpu
def test_no_two_families_share_a_scratch_slot():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    busy, alone = Engine(8, 8, 4, 0, 16), Engine(8, 8, 4, 0, 16)
    try:
        v, raw, neumf, feed, _ = _inputs(busy.device)
        enc = (v["w1"], v["b1"], v["w2"], v["b2"])
        results = []
        for e in (busy, alone):
            e.vae_encoder_load(*enc)
            indptr, nnz, thr = e.equal_sparsity_csr_begin(raw, 0.8)
            if e is busy:
                first, big, again = (_round(e, v, neumf, feed, b) for b in (33, 300, 33))
                assert len(first) == len(again) and len(big) == len(first)
                for i, (x, y) in enumerate(zip(first, again)):
                    assert x == y, f"result {i} of the b = 33 round changed after the b = 300 round"
            indices = torch.empty(max(nnz, 1), dtype=torch.int32, device=e.device)
            e.equal_sparsity_csr_end(indices)
            z, kl = e.vae_encode_csr(e.csr_to_device(feed), row0=0, b=300, return_kl=True)
            results.append(_bytes([indptr, nnz, thr, indices[:nnz], z, kl]))
            e.feed_status()
        assert 0 < nnz < raw.numel()
        for i, (x, y) in enumerate(zip(*results)):
            assert x == y, f"result {i} of begin -> end / load -> encode differs from the engine that did nothing in between"
    finally:
        busy.close()
        alone.close()
